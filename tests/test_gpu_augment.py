"""The augmentation kernels (csrc/augment.hip) behind sst_amd.augment.TrainAugment against tests/augment_ref.py, the float32
restatement that tests/test_augment_host.py pins to the reference's classes.

Rule: wherever nothing else is stated everything is EQUAL bit for bit - rows, their order, counts, offsets, boxes, labels.  The
shapes are the smallest at which the kernels can go wrong: around the wave (64) and the workgroup (256), an empty sample between
two others, every column count with its own load width, more pasted boxes than one LDS chunk holds."""
import itertools

import numpy as np
import pytest
import torch

import augment_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F = np.float32
RANGE = [-74.88, -74.88, -2, 74.88, 74.88, 4]


def _pipeline(rng=RANGE, flip=True, rst=True, shuffle=True, obj_range=True, std=(0.2, 0.2, 0.2)):
    steps = [dict(type='LoadPointsFromFile', coord_type='LIDAR', load_dim=6, use_dim=5), dict(type='ObjectSample', db_sampler=dict())]
    if flip:
        steps.append(dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5))
    if rst:
        steps.append(dict(type='GlobalRotScaleTrans', rot_range=[-0.78539816, 0.78539816], scale_ratio_range=[0.95, 1.05],
                          translation_std=list(std)))
    if rng is not None:
        steps.append(dict(type='PointsRangeFilter', point_cloud_range=list(rng)))
        if obj_range:
            steps.append(dict(type='ObjectRangeFilter', point_cloud_range=list(rng)))
    if shuffle:
        steps.append(dict(type='PointShuffle'))
    return steps + [dict(type='DefaultFormatBundle3D', class_names=['Car']), dict(type='Collect3D', keys=['points'])]


def _aug(**kw):
    from sst_amd.augment import TrainAugment
    return TrainAugment.from_pipeline(_pipeline(**kw))


def _params(batch, seed=0, **fixed):
    """drawn like a training batch (flips, angle, scale, translation, seeds), any field overridden by hand"""
    from sst_amd.augment import AugmentParams
    rs = np.random.RandomState(seed)
    p = AugmentParams(batch)
    p.flip_h, p.flip_v = rs.rand(batch) < 0.5, rs.rand(batch) < 0.5
    p.angle, p.scale = rs.uniform(-0.785, 0.785, batch), rs.uniform(0.95, 1.05, batch)
    p.trans = rs.normal(scale=0.2, size=(batch, 3))
    p.seed = rs.randint(0, 2 ** 63, batch).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    for k, v in fixed.items():
        getattr(p, k)[...] = v
    return p


def _boxes(rs, n, cols=7, spread=70.0):
    b = np.zeros((n, cols), F)
    b[:, :2] = rs.uniform(-spread, spread, (n, 2))
    b[:, 2] = rs.uniform(-1.5, 0.5, n)
    b[:, 3:6] = rs.uniform([1.5, 1.5, 1.2], [6.0, 3.0, 2.5], (n, 3))
    b[:, 6] = rs.uniform(-np.pi, np.pi, n)
    if cols == 9:
        b[:, 7:] = rs.uniform(-8, 8, (n, 2))
    return b


def _cloud(rs, n, cols, near=None):
    """points over a little more than the range; a third of them around the boxes ``near`` so that the removal has work"""
    p = np.zeros((n, cols), F)
    p[:, :3] = rs.uniform([-80, -80, -2.5], [80, 80, 4.5], (n, 3))
    if near is not None and len(near) and n:
        k = n // 3
        p[:k, :3] = near[rs.randint(0, len(near), k), :3] + rs.uniform(-3, 3, (k, 3))
    p[:, 3:] = rs.uniform(0, 1, (n, cols - 3))
    return p


def _pasted(rs, boxes, cols, per_box=7):
    """sample_all's dictionary: the boxes, labels and ``per_box`` points inside every box"""
    pts = []
    for b in boxes:
        local = rs.uniform(-0.45, 0.45, (per_box, 3)) * b[3:6]
        local[:, 2] += 0.5 * b[5]
        c, s = np.cos(b[6]), np.sin(b[6])
        p = np.zeros((per_box, cols), F)
        p[:, 0], p[:, 1] = local[:, 0] * c + local[:, 1] * s + b[0], -local[:, 0] * s + local[:, 1] * c + b[1]
        p[:, 2] = local[:, 2] + b[2]
        p[:, 3:] = rs.uniform(0, 1, (per_box, cols - 3))
        pts.append(p)
    pts = np.concatenate(pts) if pts else np.zeros((0, cols), F)
    return dict(gt_bboxes_3d=boxes, gt_labels_3d=rs.randint(0, 3, len(boxes)).astype(np.int64), points=pts)


def _bits(got, want, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape, f'{what}: shape {got.shape} vs {want.shape}'
    assert got.dtype == want.dtype, f'{what}: {got.dtype} vs {want.dtype}'
    view = np.int32 if got.dtype == np.float32 else got.dtype
    assert np.array_equal(got.view(view), want.view(view)), f'{what}: not bit for bit'


def _check(aug, points, boxes=None, labels=None, sampled=None, seed_boxes=None, params=None, on_device=False):
    """one call against the restatement, sample by sample -> (the call's result, the restatement's kept input rows per sample)"""
    batch = len(points)
    params = params if params is not None else _params(batch)
    give = [torch.from_numpy(p).to(DEV) if on_device else torch.from_numpy(p) for p in points]
    res = aug(give, boxes, labels, sampled, seed_boxes, params)
    asm = aug.assemble(boxes, labels, sampled, batch)
    rec = aug.records(params, asm)
    kept = []
    for i in range(batch):
        past = sampled[i] if sampled is not None and sampled[i] is not None else None
        rows = np.concatenate([past['points'], points[i]]) if past is not None else points[i]
        planes = R.box_planes(past['gt_bboxes_3d']) if past is not None else np.zeros((0, 6, 4), F)
        want, idx = R.augment_points(rows, 0 if past is None else past['points'].shape[0], planes, rec[i], i, aug.norm)
        _bits(res['points'][i], want, f'points of sample {i}')
        assert res['offsets'][i + 1] - res['offsets'][i] == want.shape[0]
        kept.append(idx)
        if boxes is not None:
            want_b, keep = R.transform_boxes(asm[i][0], rec[i], filter=aug.box_range is not None)
            _bits(res['gt_bboxes_3d'][i], want_b, f'boxes of sample {i}')
            _bits(res['gt_labels_3d'][i], asm[i][1][keep], f'labels of sample {i}')
        if seed_boxes is not None:
            for k, sb in enumerate(seed_boxes[i]):
                want_s, _ = R.transform_boxes(sb, rec[i], rotate=aug.rst is not None, filter=False)
                _bits(res['seed_boxes'][i][k], want_s, f'seed boxes {k} of sample {i}')
    assert res['points_packed'].shape[0] == res['offsets'][-1] == sum(len(k) for k in kept)
    return res, kept


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 255, 256, 257, 3 * 256 + 1])
def test_row_counts_around_the_wave_and_the_workgroup(n):
    rs = np.random.RandomState(n)
    pasted = _boxes(rs, 3)
    gt = _boxes(rs, 4)
    _, kept = _check(_aug(), [_cloud(rs, n, 5, pasted)], [gt], [np.arange(4) % 3], [_pasted(rs, pasted, 5)], params=_params(1, n))
    assert len(kept[0]) > 0                                         # the pasted rows at least


def test_a_batch_with_an_empty_sample_in_the_middle():
    rs = np.random.RandomState(1)
    sizes = [257, 0, 1, 1000]
    pasted = [_boxes(rs, 2), None, None, _boxes(rs, 5)]
    sampled = [_pasted(rs, b, 5) if b is not None else None for b in pasted]
    points = [_cloud(rs, n, 5, b) for n, b in zip(sizes, pasted)]
    points[2][:] = [1.0, 2.0, 0.5, 0.25, 0.75]                      # the single row of sample 2 is inside the range
    gts = [_boxes(rs, g) for g in (3, 0, 2, 65)]
    labels = [np.arange(len(g)) % 3 for g in gts]
    res, kept = _check(_aug(), points, gts, labels, sampled, params=_params(4, 5))
    assert len(kept[1]) == 0 and len(kept[2]) == 1 and res['points'][1].shape == (0, 5)
    # the empty sample has no box either: the quirk leaves it unrotated, the others are rotated
    assert res['pcd_rotation'][1] is None and all(res['pcd_rotation'][i] is not None for i in (0, 2, 3))


@pytest.mark.parametrize('cols', [3, 4, 5, 6, 8])
@pytest.mark.parametrize('on_device', [False, True])
def test_every_column_count(cols, on_device):
    rs = np.random.RandomState(cols)
    pasted = [_boxes(rs, 3), _boxes(rs, 1)]
    points = [_cloud(rs, 300, cols, pasted[0]), _cloud(rs, 77, cols, pasted[1])]
    gts = [_boxes(rs, 5), _boxes(rs, 2)]
    _check(_aug(), points, gts, [np.zeros(5, np.int64), np.ones(2, np.int64)], [_pasted(rs, b, cols) for b in pasted],
           params=_params(2, cols), on_device=on_device)


def test_unsupported_shapes_are_refused_by_name():
    aug = _aug()
    with pytest.raises(NotImplementedError, match='point columns'):
        aug([torch.zeros(4, 9)], None, None)
    with pytest.raises(NotImplementedError, match='point columns'):
        aug([torch.zeros(4, 2)], None, None)


# ------------------------------------------------------------------------------------------------ removal
def _chunk():
    from sst_amd import _lib
    return _lib.load().sst_augment_plane_chunk()


@pytest.mark.parametrize('n_boxes', [0, 1, 35, 'chunk + 6'])
def test_removal_by_pasted_boxes(n_boxes):
    """0, 1, 35 pasted boxes and more than one LDS chunk; the pasted rows lie inside their own boxes and stay"""
    s = _chunk() + 6 if n_boxes == 'chunk + 6' else n_boxes
    rs = np.random.RandomState(s)
    pasted = _boxes(rs, s, spread=40.0)
    sampled = _pasted(rs, pasted, 5, per_box=3) if s else None
    pts = _cloud(rs, 700, 5, pasted)
    if s:                                                            # rows of the cloud well inside the LAST box: past the first chunk
        pts[-20:] = _pasted(rs, pasted[-1:], 5, per_box=20)['points']
    aug = _aug(shuffle=False)
    _, kept = _check(aug, [pts], [_boxes(rs, 2)], [np.zeros(2, np.int64)], [sampled], params=_params(1, 3))
    if s:
        n_p = sampled['points'].shape[0]
        inside = R.points_in_planes(pts[:, :3], R.box_planes(pasted)).any(-1)
        assert inside[-20:].all() and 20 <= inside.sum() < 700
        assert not np.isin(n_p + np.nonzero(inside)[0], kept[0]).any()          # every own row inside a box is gone
        own_pasted = R.points_in_planes(sampled['points'][:, :3], R.box_planes(pasted)).any(-1)
        assert own_pasted.all()                                                  # the pasted rows ARE inside pasted boxes ...
        in_range = R.in_range_3d(R.transform_points(sampled['points'][:, :3], aug.records(_params(1, 3), [(0, 0, 0, True)])[0]),
                                 np.array(RANGE, F))
        assert np.array_equal(np.isin(np.arange(n_p), kept[0]), in_range)        # ... and only the range decides about them


def test_points_exactly_on_faces_are_kept():
    """dyadic boxes and points (tests/golden/augment_golden.npz): every product and sum is exact, sgn == 0 is outside"""
    from conftest import load_golden
    g = load_golden('augment_golden.npz')
    aug = _aug(flip=False, rst=False, shuffle=False)
    pts = np.concatenate([g['dyadic_points'], np.zeros((g['dyadic_points'].shape[0], 1), F)], 1)
    sampled = dict(gt_bboxes_3d=g['dyadic_boxes'], gt_labels_3d=np.zeros(3, np.int64), points=np.zeros((0, 4), F))
    _, kept = _check(aug, [pts], [np.zeros((0, 7), F)], [np.zeros(0, np.int64)], [sampled])
    inside = g['dyadic_mask'].any(-1)
    assert np.array_equal(kept[0], np.nonzero(~inside & R.in_range_3d(pts, np.array(RANGE, F)))[0])
    planes = R.box_planes(g['dyadic_boxes'])
    sgn = ((pts[:, None, None, 0] * planes[None, ..., 0] + pts[:, None, None, 1] * planes[None, ..., 1])
           + pts[:, None, None, 2] * planes[None, ..., 2]) + planes[None, ..., 3]
    on_face = ((sgn == 0).any(-1) & (sgn <= 0).all(-1)).any(-1) & ~inside & R.in_range_3d(pts, np.array(RANGE, F))
    assert on_face.sum() > 50 and np.isin(np.nonzero(on_face)[0], kept[0]).all()


def test_samples_that_lose_every_row():
    rs = np.random.RandomState(9)
    big = np.array([[0, 0, -10, 60, 60, 40, 0.3]], F)                # holds every point of sample 0
    pts0 = _cloud(rs, 300, 5)
    pts0[:, :2] = rs.uniform(-15, 15, (300, 2))
    pts1 = _cloud(rs, 200, 5)
    pts1[:, 0] += 400                                                # sample 1: outside the range, whatever the transform
    sampled = [dict(gt_bboxes_3d=big, gt_labels_3d=np.zeros(1, np.int64), points=np.zeros((0, 5), F)), None]
    res, kept = _check(_aug(), [pts0, pts1, _cloud(rs, 100, 5)], [np.zeros((0, 7), F)] * 3, [np.zeros(0, np.int64)] * 3,
                       sampled + [None], params=_params(3, 2))
    assert len(kept[0]) == 0 and len(kept[1]) == 0 and len(kept[2]) > 0
    assert res['offsets'][:3] == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ range
def test_range_bounds_are_strict_and_non_finite_rows_are_dropped():
    aug = _aug(flip=False, rst=False, shuffle=False)
    r = np.array(RANGE, F)
    rows, expect = [], []
    for k in range(3):
        for bound, inward in ((r[k], F(np.inf)), (r[k + 3], F(-np.inf))):
            on = np.array([1.0, 2.0, 0.5, 0.0], F)
            on[k] = bound
            inside = on.copy()
            inside[k] = np.nextafter(bound, inward)
            rows += [on, inside]
            expect += [False, True]
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            row = np.array([1.0, 2.0, 0.5, 0.0], F)
            row[k] = bad
            rows.append(row)
            expect.append(False)
    pts = np.stack(rows)
    pts[:, 3] = np.arange(len(rows))
    _, kept = _check(aug, [pts], None, None, None, params=_params(1, 0, flip_h=False, flip_v=False, angle=0, scale=1, trans=0))
    assert np.array_equal(kept[0], np.nonzero(expect)[0])


# ------------------------------------------------------------------------------------------------ transform
@pytest.mark.parametrize('flip_h,flip_v', list(itertools.product([False, True], repeat=2)))
def test_flip_combinations(flip_h, flip_v):
    rs = np.random.RandomState(4)
    gt = _boxes(rs, 9, cols=9)
    res, _ = _check(_aug(), [_cloud(rs, 400, 4)], [gt], [np.arange(9) % 3], None, params=_params(1, 6, flip_h=flip_h, flip_v=flip_v))
    assert res['pcd_horizontal_flip'] == [flip_h] and res['pcd_vertical_flip'] == [flip_v]


def test_a_sample_without_boxes_is_not_rotated_and_identity_keeps_the_bits():
    """the empty-box quirk (transforms_3d.py:609-614): no rotation although an angle is given; with scale 1 and translation 0
    the rows that stay are the input rows, bit for bit"""
    rs = np.random.RandomState(5)
    pts = _cloud(rs, 500, 5)
    res, kept = _check(_aug(shuffle=False), [pts], [np.zeros((0, 7), F)], [np.zeros(0, np.int64)], None,
                       params=_params(1, 1, flip_h=False, flip_v=False, angle=0.7, scale=1, trans=0))
    assert res['pcd_rotation'] == [None]
    _bits(res['points'][0], pts[kept[0]], 'identity')
    assert np.array_equal(kept[0], np.nonzero(R.in_range_3d(pts, np.array(RANGE, F)))[0])
    # with one box the same call rotates
    res, _ = _check(_aug(shuffle=False), [pts], [_boxes(rs, 1)], [np.zeros(1, np.int64)], None,
                    params=_params(1, 1, flip_h=False, flip_v=False, angle=0.7, scale=1, trans=0))
    assert res['pcd_rotation'][0] is not None


def test_normalize_points_column():
    from sst_amd.augment import TrainAugment
    steps = _pipeline()
    steps.insert(-2, dict(type='NormalizePoints'))
    rs = np.random.RandomState(8)
    pts = _cloud(rs, 300, 5)
    pts[:, 3] = rs.randint(0, 256, 300)
    _check(TrainAugment.from_pipeline(steps), [pts], [_boxes(rs, 2)], [np.zeros(2, np.int64)], None)


# ------------------------------------------------------------------------------------------------ shuffle
def test_shuffle_is_a_reproducible_permutation():
    rs = np.random.RandomState(6)
    pts = _cloud(rs, 64, 5)
    pts[:, :3] = rs.uniform(-20, 20, (64, 3)) * [1, 1, 0.05]          # all 64 rows inside the range
    gt, lab = [_boxes(rs, 2)], [np.zeros(2, np.int64)]
    p = _params(1, 7)
    shuffled, kept = _check(_aug(), [pts], gt, lab, None, params=p)
    a = shuffled['points'][0].cpu().numpy().copy()
    again, _ = _check(_aug(), [pts], gt, lab, None, params=p)
    _bits(again['points'][0], a, 'same seed')
    plain, kept_plain = _check(_aug(shuffle=False), [pts], gt, lab, None, params=p)
    b = plain['points'][0].cpu().numpy()
    assert len(kept[0]) == 64 and np.array_equal(kept_plain[0], np.arange(64)) and not np.array_equal(kept[0], kept_plain[0])
    assert np.array_equal(np.sort(kept[0]), kept_plain[0])
    assert np.array_equal(a, b[kept[0]])                             # a permutation of the unshuffled output
    p2 = _params(1, 7)
    p2.seed[0] += np.uint64(2)
    other, kept2 = _check(_aug(), [pts], gt, lab, None, params=p2)
    assert not np.array_equal(kept2[0], kept[0]) and np.array_equal(np.sort(kept2[0]), np.arange(64))


def test_shuffle_orders_are_uniform():
    """one call, one seed, 2 400 samples of 4 in-range rows: each of the 24 orders occurs between 50 and 150 times (expected
    100, standard deviation 9.8: the bound is 5 sigma).  The sample field of the key holds 2^31 - 1 samples."""
    from sst_amd.augment import AugmentParams
    batch = 2400
    aug = _aug(flip=False, rst=False)
    pts = np.zeros((4, 4), F)
    pts[:, 0], pts[:, 3] = [1, 2, 3, 4], [0, 1, 2, 3]
    p = AugmentParams(batch)
    p.seed[:] = np.uint64(0x0123456789ABCDEF)
    res = aug([torch.from_numpy(pts)] * batch, None, None, None, None, p)
    assert res['offsets'] == list(range(0, 4 * batch + 1, 4))
    order = res['points_packed'][:, 3].cpu().numpy().astype(np.int64).reshape(batch, 4)
    assert (np.sort(order, 1) == np.arange(4)).all()
    for s in (0, 1, 1234, batch - 1):                                # the exact order of a few samples against the restatement
        assert np.array_equal(order[s], np.argsort(R.shuffle_keys(p.seed[s], s, 4), kind='stable'))
    counts = np.bincount(order @ np.array([64, 16, 4, 1]), minlength=256)
    counts = counts[counts > 0]
    print('orders:', len(counts), 'min', counts.min(), 'max', counts.max())
    assert len(counts) == 24 and counts.min() >= 50 and counts.max() <= 150


# ------------------------------------------------------------------------------------------------ boxes
@pytest.mark.parametrize('cols', [7, 9])
def test_box_counts_and_columns(cols):
    """0, 1 and 65 boxes per sample (more than a wave, the ranks cross wave boundaries), some centres outside the BEV range;
    D = 9: the velocity columns follow both flips, the rotation and the scale"""
    rs = np.random.RandomState(cols)
    gts = [_boxes(rs, g, cols, spread=90.0) for g in (0, 1, 65)]
    labels = [rs.randint(0, 3, len(g)).astype(np.int64) for g in gts]
    seeds = [[_boxes(rs, 3, cols, spread=120.0), _boxes(rs, 0, cols)], [_boxes(rs, 1, cols, spread=120.0)], [_boxes(rs, 70, cols, spread=120.0)]]
    p = _params(3, 11, flip_h=[True, False, True], flip_v=[False, True, True])
    res, _ = _check(_aug(), [_cloud(rs, 50, 5)] * 3, gts, labels, None, seeds, params=p)
    assert 0 < res['gt_bboxes_3d'][2].shape[0] < 65 and res['gt_bboxes_3d'][0].shape == (0, cols)
    assert res['seed_boxes'][2][0].shape == (70, cols) and len(res['seed_boxes'][0]) == 2      # seed boxes are never filtered
    assert res['gt_labels_3d'][2].dtype == torch.int64 and res['gt_bboxes_3d'][2].is_cuda


def test_yaw_on_plus_minus_pi_and_centres_on_the_bev_bound():
    r = np.array(RANGE, F)
    pi = F(np.pi)
    gt = np.array([[1, 1, 0, 4, 2, 1.5, pi], [2, 2, 0, 4, 2, 1.5, -pi], [3, 3, 0, 4, 2, 1.5, 0.0],      # the last: yaw = pi after flip_h
                   [r[0], 0, 0, 4, 2, 1.5, 0.1], [r[3], 0, 0, 4, 2, 1.5, 0.1], [0, r[1], 0, 4, 2, 1.5, 0.1], [0, r[4], 0, 4, 2, 1.5, 0.1],
                   [np.nextafter(r[0], F(0)), np.nextafter(r[4], F(0)), 0, 4, 2, 1.5, 0.1]], F)
    ident = dict(angle=0, scale=1, trans=0)
    aug = _aug()
    for flip_h in (False, True):
        res, _ = _check(aug, [np.zeros((1, 4), F)], [gt], [np.arange(8)], None, params=_params(1, 0, flip_h=flip_h, flip_v=False, **ident))
        got = res['gt_bboxes_3d'][0].cpu().numpy()
        want_labels = [0, 1, 2, 7]
        assert res['gt_labels_3d'][0].tolist() == want_labels           # the four centres on a bound are dropped, the one inside stays
        assert np.all(np.abs(got[:, 6]) <= pi)
        # yaw exactly +pi before limit_yaw: pi / (2 pi) + 0.5 = 1 exactly, floor 1, pi - 2 pi = -pi; -pi stays -pi
        if not flip_h:
            assert got[0, 6] == -pi and got[1, 6] == -pi
        else:
            assert got[2, 6] == -pi                                     # -0 + (float)pi = pi, then as above


# ------------------------------------------------------------------------------------------------ the golden of the host test
def test_golden_end_to_end_through_the_kernels():
    """the assertions tests/test_augment_host.py makes of the restatement, made of the kernels: the reference's kept rows in its
    order, kept boxes and labels, x and y within the propagated rotation bar, everything else bit for bit"""
    import test_augment_host as H
    g = R.load_golden(GOLDEN)
    aug = _aug(shuffle=False)
    from sst_amd.augment import AugmentParams
    for fh, fv in itertools.product((0, 1), repeat=2):
        runs = [R.golden_run(g, fh, fv, si) for si in (0, 1)]
        p = AugmentParams(2)
        for i, r in enumerate(runs):
            p.flip_h[i], p.flip_v[i], p.angle[i], p.scale[i], p.trans[i] = fh, fv, r['angle'], r['scale'], r['trans']
        sampled = [dict(gt_bboxes_3d=r['pasted'], gt_labels_3d=r['pasted_labels'], points=r['pasted_points']) for r in runs]
        res, kept = _check(aug, [r['in_points'] for r in runs], [r['in_gt'] for r in runs], [r['in_gt_labels'] for r in runs],
                           sampled, params=p)
        for i, r in enumerate(runs):
            assert np.array_equal(kept[i], r['s0_rows'][r['point_mask']])
            out = res['points'][i].cpu().numpy()
            want = np.concatenate([r['s4_points'], r['s0_points'][:, 3:]], 1)[r['point_mask']]
            tol = (1.05 * H.ROT_BAR_ULP * H._ulp(np.abs(r['s1_points'][:, 0]) + np.abs(r['s1_points'][:, 1]))
                   + H._ulp(r['s3_points'][:, :2]).max(1) + H._ulp(r['s4_points'][:, :2]).max(1))[r['point_mask']]
            assert out.shape == want.shape and (np.abs(out[:, :2].astype(np.float64) - want[:, :2]) <= tol[:, None]).all()
            assert np.array_equal(out[:, 2:], want[:, 2:])
            boxes = res['gt_bboxes_3d'][i].cpu().numpy()
            assert np.array_equal(res['gt_labels_3d'][i].cpu().numpy(), r['s5_labels']) and boxes.shape == r['s5_boxes'].shape
            tol = (1.05 * H.ROT_BAR_ULP * H._ulp(np.abs(r['s1_boxes'][:, 0]) + np.abs(r['s1_boxes'][:, 1]))
                   + H._ulp(r['s3_boxes'][:, :2]).max(1) + H._ulp(r['s4_boxes'][:, :2]).max(1))[r['box_mask']]
            assert (np.abs(boxes[:, :2].astype(np.float64) - r['s5_boxes'][:, :2]) <= tol[:, None]).all()
            assert np.array_equal(boxes[:, 2:], r['s5_boxes'][:, 2:])
            assert np.array_equal(res['pcd_rotation'][i].numpy(), r['rot_mat_T'])


# ------------------------------------------------------------------------------------------------ into a detector, steady state
def test_one_training_step_takes_the_output():
    """a small SST detector from the shipped model dictionary, heads attached, takes the views, boxes and labels as they come"""
    import test_gpu_sst_detector as D
    det = D._build('DynamicVoxelNet')
    rs = np.random.RandomState(2)
    half = D.HALF
    aug = _aug(rng=[-half, -half, -2, half, half, 4])
    points, gts, labels = [], [], []
    for n in (2500, 2100):
        p = np.zeros((n, 3), F)
        p[:] = rs.uniform([-half - 1, -half - 1, -1.9], [half + 1, half + 1, 1.0], (n, 3))
        b = _boxes(rs, 4, spread=half - 2)
        b[:, 2] = -1.8
        points.append(torch.from_numpy(p))
        gts.append(b)
        labels.append(np.array([0, 1, 2, 0]))
    res = aug(points, gts, labels)
    assert all(0 < p.shape[0] < n for p, n in zip(res['points'], (2500, 2100)))
    losses = det.forward_train(res['points'], [{}] * 2, res['gt_bboxes_3d'], res['gt_labels_3d'])
    flat = [v for val in losses.values() for v in (val if isinstance(val, (list, tuple)) else [val])]
    assert flat and all(bool(torch.isfinite(v).all()) for v in flat)


@pytest.mark.parametrize('on_device', [False, True])
def test_later_calls_allocate_nothing_on_the_device(on_device):
    rs = np.random.RandomState(3)
    aug = _aug()
    pasted = [_boxes(rs, 4), _boxes(rs, 2)]
    sampled = [_pasted(rs, b, 5) for b in pasted]
    gts, labels = [_boxes(rs, 6), _boxes(rs, 3)], [np.zeros(6, np.int64), np.zeros(3, np.int64)]
    seeds = [[_boxes(rs, 2)], [_boxes(rs, 1)]]
    allocs = []
    for it in range(3):
        points = [torch.from_numpy(_cloud(rs, n, 5, b)) for n, b in zip((900, 700), pasted)]
        if on_device:
            points = [p.to(DEV) for p in points]
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()['allocation.all.allocated']
        res = aug(points, gts, labels, sampled, seeds, _params(2, it))
        torch.cuda.synchronize()
        allocs.append(torch.cuda.memory_stats()['allocation.all.allocated'] - before)
        assert res['points_packed'].shape[0] > 0
    assert allocs[0] > 0 and allocs[1:] == [0, 0]
