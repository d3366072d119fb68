"""GPU: furthest point sampling, the SSG assignment and the SSG / hybrid assigners (csrc/fps.hip) - exact against the numpy
float32 restatements of tests/fps_ref.py (pinned to the reference by tests/test_fps_host.py) and against the reference's own
outputs in tests/golden/ssg.npz."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fps_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def random_points(n, seed):
    return (np.random.default_rng(seed).standard_normal((n, 3)) * 10).astype(np.float32)


def sample_counts(n):
    return sorted({1, 2, min(n, 512)} | ({n} if n <= 1025 else set()))


# sizes around every storage tier of the kernel (1 | 2 | 4 | 8 | 16 points per thread in registers, then streamed)
PLAIN_SIZES = [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 1500, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385]


@pytest.mark.parametrize('n', PLAIN_SIZES)
def test_fps_random_points(n):
    import sst_amd
    pts = random_points(n, n)
    want = R.fps(pts, max(sample_counts(n)))       # the samples of a shorter call are a prefix of a longer one's
    for m in sample_counts(n):
        got = sst_amd.furthest_point_sample(dev(pts)[None], m)
        assert got.dtype == torch.int32 and tuple(got.shape) == (1, m)
        np.testing.assert_array_equal(host(got)[0], want[:m])


def test_fps_streamed_tier():
    import sst_amd
    pts = random_points(70000, 7)
    got = sst_amd.furthest_point_sample(dev(pts)[None], 256)
    np.testing.assert_array_equal(host(got)[0], R.fps(pts, 256))


@pytest.mark.parametrize('n', [5, 37, 100, 1500, 3000, 6000, 12000, 16000, 20000])
def test_fps_lattice_points_follow_the_tie_rule(n):
    """integer-lattice points: exact ties at every sample; a non-power-of-two n in every tier (fewer threads than points in
    the reference's launch).  Once all lattice sites are taken every distance is 0 and point 0 must win."""
    import sst_amd
    pts = R.lattice(n, seed=n, side=6)
    m = min(n, 300)
    want = R.fps(pts, m)
    np.testing.assert_array_equal(host(sst_amd.furthest_point_sample(dev(pts)[None], m))[0], want)
    if n >= 1500:
        assert (want[-20:] == 0).all()
        assert (want != R.fps(pts, m, rank=R.lowest_index_rank(n))).any()       # the case tells the two rules apart


def test_fps_identical_points_and_more_samples_than_points():
    import sst_amd
    same = np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (700, 1))
    assert (host(sst_amd.furthest_point_sample(dev(same)[None], 40)) == 0).all()
    pts = random_points(5, 3)
    got = host(sst_amd.furthest_point_sample(dev(pts)[None], 9))[0]
    np.testing.assert_array_equal(got, R.fps(pts, 9))
    assert (got[5:] == 0).all()


def test_fps_batches_and_input_checks():
    import sst_amd
    pts = np.stack([random_points(1300, s) for s in (1, 2, 3)])
    got = host(sst_amd.furthest_point_sample(dev(pts), 64))
    for b in range(3):
        np.testing.assert_array_equal(got[b], R.fps(pts[b], 64))
    assert tuple(sst_amd.furthest_point_sample(dev(pts), 0).shape) == (3, 0)
    with pytest.raises(RuntimeError):
        sst_amd.furthest_point_sample(dev(pts).transpose(0, 1), 4)             # not contiguous
    with pytest.raises(RuntimeError):
        sst_amd.furthest_point_sample(dev(pts).double(), 4)
    with pytest.raises(RuntimeError):
        sst_amd.furthest_point_sample(dev(pts)[..., :2], 4)


def test_fps_segmented():
    """segments of lengths 0, 1, 5, 64, 1025 and 20 000 in one call (empty, register tiers, streamed tier), read from a
    strided [N, 5] array; each segment equals the plain call on that segment alone"""
    import sst_amd
    lengths = [0, 1, 5, 64, 1025, 20000, 0, 300]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    wide = np.random.default_rng(4).standard_normal((offsets[-1], 5)).astype(np.float32)
    pts = wide[:, :3]
    view = dev(wide)[:, :3]
    assert view.stride(0) == 5
    m = 70
    for flag in (False, True):
        idx, count = sst_amd.fps_segmented(view, dev(offsets), m, identity_if_short=flag)
        idx, count = host(idx), host(count)
        np.testing.assert_array_equal(count, [0 if n == 0 else (min(n, m) if flag else m) for n in lengths])
        for s, n in enumerate(lengths):
            if n == 0:
                assert (idx[s] == -1).all()
            elif flag and n <= m:
                np.testing.assert_array_equal(idx[s], np.concatenate([np.arange(n), np.full(m - n, -1)]))
            else:
                seg = np.ascontiguousarray(pts[offsets[s]:offsets[s + 1]])
                np.testing.assert_array_equal(idx[s], R.fps(seg, m))
                np.testing.assert_array_equal(idx[s], host(sst_amd.furthest_point_sample(dev(seg)[None], m))[0])
    idx, count = sst_amd.fps_segmented(view, dev(offsets), 0)
    assert tuple(idx.shape) == (len(lengths), 0)
    idx, count = sst_amd.fps_segmented(view, dev(offsets[:1]), 5)
    assert tuple(idx.shape) == (0, 5) and count.numel() == 0


@pytest.mark.parametrize('n', [5, 100, 1025])
def test_fps_with_dist(n):
    import sst_amd
    pts = np.stack([random_points(n, n), R.lattice(n, n + 1, side=5)])
    d = pts[:, :, None, :] - pts[:, None, :, :]
    mat = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float32)   # the kernel's arithmetic
    m = min(n, 200)
    got = host(sst_amd.furthest_point_sample_with_dist(dev(mat), m))
    plain = host(sst_amd.furthest_point_sample(dev(pts), m))
    for b in range(2):
        np.testing.assert_array_equal(got[b], R.fps_with_dist(mat[b], m))
        np.testing.assert_array_equal(got[b], plain[b])
    with pytest.raises(RuntimeError):
        sst_amd.furthest_point_sample_with_dist(dev(mat)[:, :, :-1], 2)


def test_fps_with_dist_streamed_tier():
    import sst_amd
    n = 16500
    mat = torch.rand((1, n, n), device=DEV, generator=torch.Generator(DEV).manual_seed(9))

    class Rows(object):          # the restatement reads one row per sample: the matrix stays on the device
        def __len__(self):
            return n

        def __getitem__(self, i):
            return host(mat[0, i])

    got = host(sst_amd.furthest_point_sample_with_dist(mat, 12))[0]
    np.testing.assert_array_equal(got, R.fps_with_dist(Rows(), 12))


# ----------------------------------------------------------------------------------------------------------------------
# sst_ssg_assign_f32 on given keypoints
# ----------------------------------------------------------------------------------------------------------------------
def run_assign(pts, offsets, key_idx, key_count, thr2, radius):
    import sst_amd
    ids, n_clusters, status = sst_amd.ssg_assign(dev(np.asarray(pts, np.float32)), dev(np.asarray(offsets, np.int32)),
                                                 dev(np.asarray(key_idx, np.int32)), dev(np.asarray(key_count, np.int32)),
                                                 thr2, radius)
    return host(ids), int(n_clusters), int(status)


def test_ssg_assign_equals_restatement_on_three_segments():
    """clustered points, more keypoints than a tile (256) in one segment, an empty segment in the middle; the ids run on
    from segment to segment"""
    import sst_amd
    lengths = [900, 0, 2500, 40]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    pts, _ = R.quantised_clusters(int(offsets[-1]), 80, 0.4, 1, seed=21)
    m = 600
    key_idx, key_count = sst_amd.fps_segmented(dev(pts), dev(offsets), m, identity_if_short=True)
    want_idx, want_count = R.fps_segmented(pts, offsets, m, True)
    np.testing.assert_array_equal(host(key_idx), want_idx)
    np.testing.assert_array_equal(host(key_count), want_count)
    radius = 1.0
    ids, n_clusters, status = run_assign(pts, offsets, want_idx, want_count, radius * 2 + 0.01, radius)
    want = R.ssg_assign(pts, offsets, want_idx, want_count, np.float32(radius * 2 + 0.01), np.float32(radius))
    np.testing.assert_array_equal(ids, want[0])
    assert (n_clusters, status) == (want[1], want[2]) and status == 0
    first_of_last = ids[offsets[3]:][ids[offsets[3]:] >= 0].min()
    assert first_of_last > ids[:offsets[3]].max()                 # the numbering base carries across the segments


def test_ssg_assign_pruning_is_any_earlier_and_the_ball_is_open():
    # keypoints 0, 3, 6 on a line, thr2 = 4.01: 1 falls to 0 and 2 falls to the fallen 1 (a greedy filter keeps 2)
    pts = np.array([[0, 0, 0], [3, 0, 0], [6, 0, 0], [2, 0, 0], [1.5, 0, 0]], np.float32)
    ids, n_clusters, status = run_assign(pts, [0, 5], [[0, 1, 2]], [3], 4.01, 2.0)
    # the point at distance exactly 2.0 = radius is outside (strict <), the one at 1.5 inside
    assert list(ids) == [0, -1, -1, -1, 0] and n_clusters == 1 and status == 0
    want = R.ssg_assign(pts, [0, 5], [[0, 1, 2]], [3], 4.01, 2.0)
    assert list(want[0]) == list(ids) and want[1:] == (1, 0)
    # every keypoint but the first pruned: one cluster, numbering base moves by one
    pts2 = np.concatenate([np.random.default_rng(1).uniform(-0.5, 0.5, (50, 3)), [[10, 10, 0]]]).astype(np.float32)
    offs = [0, 50, 51]
    keys = np.full((2, 50), -1, np.int32)
    keys[0] = np.arange(50)
    keys[1, 0] = 0
    ids, n_clusters, status = run_assign(pts2, offs, keys, [50, 1], 4.01, 2.0)
    assert (ids[:50] == 0).all() and ids[50] == 1 and n_clusters == 2 and status == 0


def test_ssg_assign_status_bits_and_empty_input():
    from sst_amd import fps as F
    pts = np.array([[0, 0, 0], [1, 0, 0], [0.5, 0, 0]], np.float32)
    # thr2 = 0 skips the pruning: both keypoints stand 1 apart with balls of radius 2 -> every point in two balls
    ids, n_clusters, status = run_assign(pts, [0, 3], [[0, 1]], [2], 0.0, 2.0)
    assert (ids == -1).all() and n_clusters == 2 and status == F.SSG_MULTI_BALL | F.SSG_EMPTY_SEGMENT
    assert R.ssg_assign(pts, [0, 3], [[0, 1]], [2], 0.0, 2.0)[2] == status
    with pytest.raises(AssertionError):
        F.raise_on_status(status)
    # a keypoint index outside its segment is skipped and reported
    ids, n_clusters, status = run_assign(pts, [0, 3], [[0, 7]], [2], 4.01, 2.0)
    assert (ids == 0).all() and n_clusters == 1 and status == F.SSG_BAD_KEYPOINT
    ids, n_clusters, status = run_assign(np.zeros((0, 3), np.float32), [0], np.zeros((0, 4), np.int32), np.zeros(0, np.int32), 4.01, 2.0)
    assert ids.size == 0 and n_clusters == 0 and status == 0


# ----------------------------------------------------------------------------------------------------------------------
# ssg and the assigners
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(R.FAMILIES))
def test_ssg_reproduces_the_reference(name):
    import sst_amd
    g = load_golden('ssg.npz')
    _, _, num_fps, radius = R.family(name)
    pts, batch = g[f'{name}_points'], g[f'{name}_batch']
    got = sst_amd.ssg(dev(pts), dev(batch), num_fps, radius)
    assert got.dtype == torch.int64
    np.testing.assert_array_equal(host(got), g[f'{name}_ssg'])
    one = np.ascontiguousarray(pts[batch == 0])
    np.testing.assert_array_equal(host(sst_amd.ssg_single_sample(dev(one), num_fps, radius)), R.ssg(one, np.zeros(len(one), int), num_fps, radius)[0])
    k = min(num_fps, len(one))
    from sst_amd import cluster
    np.testing.assert_array_equal(host(cluster.fps(dev(one), k)), one[R.fps(one, k)])


def test_ssg_unsorted_samples_and_repeats():
    import sst_amd
    pts, batch = R.quantised_clusters(4000, 60, 0.3, 2, seed=31)
    want, status = R.ssg(pts, batch, 256, 1.0)
    assert status == 0
    got = host(sst_amd.ssg(dev(pts), dev(batch), 256, 1.0))
    np.testing.assert_array_equal(got, want)
    perm = np.random.default_rng(2).permutation(len(pts))
    shuffled = host(sst_amd.ssg(dev(pts[perm]), dev(batch[perm]), 256, 1.0))
    # a stable sort by sample keeps the shuffled order inside a sample: the restatement on that order is the answer
    order = np.argsort(batch[perm], kind='stable')
    want_sorted, _ = R.ssg(pts[perm][order], batch[perm][order], 256, 1.0)
    back = np.empty_like(want_sorted)
    back[order] = want_sorted
    np.testing.assert_array_equal(shuffled, back)
    for _ in range(3):
        np.testing.assert_array_equal(host(sst_amd.ssg(dev(pts), dev(batch), 256, 1.0)), got)
    assert sst_amd.ssg(dev(pts[:0]), dev(batch[:0]), 256, 1.0).numel() == 0


def _assigners():
    import sst_amd
    a, b = sst_amd.SSGAssigner(**copy.deepcopy(R.SSG_ASSIGNER)), sst_amd.HybridAssigner(**copy.deepcopy(R.HYBRID_ASSIGNER))
    return {'ssgassigner': a, 'hybrid': b}


@pytest.mark.parametrize('tag', ['ssgassigner', 'hybrid'])
def test_assigners_reproduce_the_reference(tag):
    g = load_golden('ssg.npz')
    module = _assigners()[tag]
    points, batches = [], []
    for class_name, fam in R.CLASS_FAMILY.items():
        pts, batch = dev(g[f'{fam}_points']), dev(g[f'{fam}_batch'])
        points.append(pts)
        batches.append(batch)
        rows, mask = module.forward_single_class(pts, batch, class_name, None)
        assert rows.dtype == torch.int64 and mask.dtype == torch.bool
        np.testing.assert_array_equal(host(rows), g[f'{tag}_{class_name}_rows'])
        np.testing.assert_array_equal(host(mask), g[f'{tag}_{class_name}_mask'])
    rows_list, mask_list = module(points, batches)
    for i, class_name in enumerate(R.CLASS_FAMILY):
        np.testing.assert_array_equal(host(rows_list[i])[:, 1:], g[f'{tag}_{class_name}_rows'])
        assert (host(rows_list[i])[:, 0] == i).all()
        np.testing.assert_array_equal(host(mask_list[i]), g[f'{tag}_{class_name}_mask'])


@pytest.mark.parametrize('tag', ['ssgassigner', 'hybrid'])
def test_assigners_equal_the_restated_flow(tag):
    """a 4 000-point, two-sample set with coordinates in multiples of 1/64 (exact voxel sums), per point; three repeats are
    bit-identical; an empty class gives empty outputs"""
    module = _assigners()[tag]
    pts, batch = R.quantised_clusters(4000, 60, 0.3, 2, seed=41)
    for class_name in R.CLASS_FAMILY:
        if tag == 'ssgassigner':
            c = R.SSG_ASSIGNER
            want = R.ssg_assigner_single_class(pts, batch, c['cluster_voxel_size'][class_name], R.PC_RANGE,
                                               c['num_fps'][class_name], c['radius'][class_name], per_sample=False)
        else:
            c = R.HYBRID_ASSIGNER['cfg_per_class'][class_name]
            if c['assigner_type'] == 'ssg':
                want = R.ssg_assigner_single_class(pts, batch, c['cluster_voxel_size'], R.PC_RANGE, c['num_fps'], c['radius'],
                                                   per_sample=True)
            else:
                want = R.ccl_assigner_single_class(pts, batch, c['cluster_voxel_size'], R.PC_RANGE, c['min_points'],
                                                   c['connected_dist'])
        first = None
        for _ in range(3):
            rows, mask = module.forward_single_class(dev(pts), dev(batch), class_name, None)
            np.testing.assert_array_equal(host(rows), want[0])
            np.testing.assert_array_equal(host(mask), want[1])
            first = first if first is not None else host(rows)
            np.testing.assert_array_equal(host(rows), first)
        rows, mask = module.forward_single_class(dev(pts[:0]), dev(batch[:0]), class_name, None)
        assert tuple(rows.shape) == (0, 2) and mask.numel() == 0


def test_shim_fills_the_callers_tensors():
    import sst_amd
    import sst_amd.native_shims as shims
    pts = dev(np.stack([random_points(1500, 1), random_points(1500, 2)]))
    b, n, m = 2, 1500, 48
    out = torch.zeros((b, m), dtype=torch.int32, device=DEV)
    temp = torch.full((b, n), 1e10, dtype=torch.float32, device=DEV)
    shims.furthest_point_sample_ext.furthest_point_sampling_wrapper(b, n, m, pts, temp, out)
    assert torch.equal(out, sst_amd.furthest_point_sample(pts, m))
    mat = ((pts[0][:, None] - pts[0][None]) ** 2).sum(-1)[None].contiguous()
    out1 = torch.zeros((1, m), dtype=torch.int32, device=DEV)
    shims.furthest_point_sample_ext.furthest_point_sampling_with_dist_wrapper(1, n, m, mat, temp[:1].contiguous(), out1)
    assert torch.equal(out1, sst_amd.furthest_point_sample_with_dist(mat, m))
    with pytest.raises(RuntimeError):      # shapes are checked before any launch
        shims.furthest_point_sample_ext.furthest_point_sampling_wrapper(b, n + 1, m, pts, temp, out)
    with pytest.raises(RuntimeError):
        shims.furthest_point_sample_ext.furthest_point_sampling_wrapper(b, n, m, pts, temp, out[:, :-1])
