"""The tracklet pipeline kernels (csrc/tracklet_augment.hip, and csrc/augment.hip's box kernel behind them) through
sst_amd.tracklet_augment.TrackletAugment against tests/tracklet_augment_ref.py, the float32 restatement that
tests/test_tracklet_augment_host.py pins to the reference's classes.

Rule: wherever nothing else is stated everything is EQUAL bit for bit - rows, their order, frame indices, counts, boxes.  The
host side of a call (the cut, the frame matrices, the noise, the decoration values: sst_amd.tracklet_augment.prepare_boxes, pinned
by the host test) feeds both sides.  The shapes are the smallest at which the kernels can go wrong: frames around the wave (64)
and the workgroup (256) and across their boundaries, 1 to 201 frames, a sample of empty frames between two others, every pair
of column counts with its own path."""
import copy
import itertools

import numpy as np
import pytest
import torch

import tracklet_augment_ref as R
import tracklet_ref as T
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F = np.float32
RANGE = [-24.0, -24.0, -2.5, 24.0, 24.0, 3.0]
PROPS = {0: [], 1: ['yaw'], 3: ['size'], 5: ['yaw', 'size', 'score'], 6: ['yaw', 'size', 'score', 'length'],
         8: ['size', 'yaw', 'size', 'score']}


def _pipeline(train=True, deco=5, rng=RANGE, shuffle=True, cut=None, cons=False, use_dim=None):
    steps = [dict(type='LoadTrackletPoints', load_dim=6, use_dim=use_dim, max_points=1024)]
    if train:
        steps.append(dict(type='LoadTrackletAnnotations'))
        if cut is not None:
            steps.append(dict(type='TrackletCutting', **cut))
    steps.append(dict(type='TrackletPoseTransform', concat=False))
    if train:
        steps.append(dict(type='TrackletNoise', center_noise_cfg=dict(max_noise=[0.2, 0.2, 0.1], consistent=cons),
                          size_noise_cfg=dict(max_noise=[0.2, 0.2, 0.1], consistent=cons), yaw_noise_cfg=dict(max_noise=0.2, consistent=False)))
    steps.append(dict(type='PointDecoration', properties=PROPS[deco], concat=True))
    if train:
        steps += [dict(type='TrackletRandomFlip', flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
                  dict(type='TrackletGlobalRotScaleTrans', rot_range=[-0.78539816, 0.78539816], scale_ratio_range=[0.95, 1.05],
                       translation_std=[0, 0, 0.2])]
    if rng is not None:
        steps.append(dict(type='PointsRangeFilter', point_cloud_range=list(rng)))
    if shuffle:
        steps.append(dict(type='PointShuffle'))
    return steps + [dict(type='TrackletFormatBundle', class_names=['Car']), dict(type='Collect3D', keys=['points'])]


def _aug(**kw):
    from sst_amd.tracklet_augment import TrackletAugment
    return TrackletAugment.from_pipeline(_pipeline(**kw))


def _pose(rs, k, identity=False):
    m = np.eye(4, dtype=F)
    if not identity:
        a = 0.3 + 0.004 * k
        m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        m[:3, 3] = [1.0e4 + 1.1 * k, -2.0e4 + 0.4 * k, 30 + 0.01 * k]
    return m


def _tracklet(rs, n, n_cands=0, identity=False, name='t'):
    """a tracklet of n frames near the ego vehicle with rigid world poses, and candidates on a subset of its frames plus two
    frames outside it"""
    import sst_amd
    boxes = T.track_boxes(np.random.default_rng(rs.randint(1 << 30)), n + 2, 0)
    boxes[:, :2] *= 0.2
    ts = [T.TS0 + 100_000 * k for k in range(n + 2)]
    poses = [torch.as_tensor(_pose(rs, k, identity)) for k in range(n + 2)]
    trk = sst_amd.LiDARTracklet('seg', name, 0, True, torch.as_tensor(boxes[:n].copy()), ts[:n], rs.uniform(0.1, 0.9, n).astype(F).tolist())
    trk.freeze()
    trk.set_type(0, 'mmdet3d')
    trk.pose_list = poses[:n]
    cands = []
    for c in range(n_cands):
        keep = sorted(set(np.nonzero(rs.rand(n) < 0.7)[0].tolist()) | {0}) + [n, n + 1]
        g = sst_amd.LiDARTracklet('seg', f'{name}g{c}', 0, True, torch.as_tensor(T.jitter(np.random.default_rng(c), boxes[keep], 0.5 * c)),
                                  [ts[i] for i in keep], [1.0] * len(keep))
        g.freeze()
        g.set_type(0, 'mmdet3d')
        g.pose_list = [poses[i] for i in keep]
        cands.append(g)
    return trk, cands


def _frames(rs, trk, lens, cols, spread=(30.0, 30.0, 3.5)):
    out = []
    for k, m in enumerate(lens):
        p = np.zeros((m, cols), F)
        p[:, :3] = trk.boxes[k, :3].numpy() + rs.uniform(-1, 1, (m, 3)) * spread
        p[:, 3:] = rs.uniform(0, 1, (m, cols - 3))
        out.append(p)
    return out


def _params(aug, trks, seed=0, **fixed):
    p = aug.draw_params(trks, np.random.RandomState(seed), torch.Generator().manual_seed(seed))
    p.seed = p.seed | np.uint64(1)
    for k, v in fixed.items():
        getattr(p, k)[...] = v
    return p


def _bits(got, want, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape, f'{what}: shape {got.shape} vs {want.shape}'
    assert got.dtype == want.dtype, f'{what}: {got.dtype} vs {want.dtype}'
    view = np.int32 if got.dtype == np.float32 else got.dtype
    assert np.array_equal(got.view(view), want.view(view)), f'{what}: not bit for bit'


def _check(aug, frames, trks, cands=None, params=None, give=None):
    """one call against the restatement, sample by sample -> (the call's result, the kept input rows per sample (indices into
    the rows of the kept frames), the host preparation)"""
    batch = len(trks)
    params = params if params is not None else _params(aug, trks)
    host_t, host_c = copy.deepcopy(trks), copy.deepcopy(cands)
    per_sample, boxes, ranges = aug.prepare_boxes(host_t, host_c, params)
    rec = aug.records(params)
    res = aug(give if give is not None else frames, trks, cands, params)
    kept = []
    for i in range(batch):
        mm, deco, values, (head, n), center = per_sample[i]
        want, fi, idx = R.augment_sample(frames[i][head:head + n], mm.numpy(), deco.numpy(), values, rec[i], i)
        _bits(res['points'][i], want, f'points of sample {i}')
        _bits(res['pts_frame_inds'][i], fi, f'frame indices of sample {i}')
        assert res['counts'][i] == want.shape[0] == res['offsets'][i + 1] - res['offsets'][i]
        kept.append(idx)
        members = [trks[i]] + list(cands[i] if cands is not None else [])
        for m, (r0, r1) in zip(members, ranges[i]):
            want_b, _ = R.transform_boxes(boxes[r0:r1].numpy(), rec[i], rotate=aug.rst is not None, filter=False)
            _bits(m.boxes, want_b, f'boxes of sample {i}')
            assert m.boxes.is_cuda and m.boxes.data_ptr() == res['boxes_packed'][r0:r1].data_ptr() and len(m) == r1 - r0
            assert torch.equal(m.shared_pose, center)
        assert (getattr(trks[i], 'rot_angle', None) == float(params.angle[i])) == (aug.rst is not None)
    assert res['points_packed'].shape[0] == res['offsets'][-1] == sum(len(k) for k in kept)
    return res, kept, per_sample


# ------------------------------------------------------------------------------------------------ sizes
def test_rows_per_frame_around_the_wave_and_the_workgroup():
    """frames of 0, 1, 63, 64, 65, 255, 256 and 257 rows in one sample: their rows straddle workgroup boundaries at 256, 512,
    768; a second sample starts in a workgroup of its own"""
    rs = np.random.RandomState(0)
    lens = [[0, 1, 63, 64, 65, 255, 256, 257, 0, 3], [257, 0, 0, 65]]
    trks, cands = zip(*[_tracklet(rs, len(n), 1, name=f't{i}') for i, n in enumerate(lens)])
    frames = [_frames(rs, t, n, 5) for t, n in zip(trks, lens)]
    aug = _aug()
    _, kept, _ = _check(aug, frames, list(trks), [list(c) for c in cands])
    assert all(0 < len(k) < sum(n) for k, n in zip(kept, lens))


@pytest.mark.parametrize('n_frames', [1, 2, 200, 201])
def test_frame_counts(n_frames):
    rs = np.random.RandomState(n_frames)
    trk, cands = _tracklet(rs, n_frames, 2)
    lens = rs.randint(0, 6, n_frames)
    lens[0] = 3
    other, other_c = _tracklet(rs, 3, 0, name='o')
    frames = [_frames(rs, trk, lens, 5), _frames(rs, other, [2, 0, 7], 5)]
    aug = _aug(cut=dict(ratio=0.0, max_length=150))
    res, kept, per_sample = _check(aug, frames, [trk, other], [cands, other_c], _params(aug, [trk, other], n_frames))
    assert len(kept[0]) > 0 and (per_sample[0][3][1] == 150) == (n_frames > 150)         # 200 and 201 frames are cut to 150


def test_a_sample_of_empty_frames_in_the_middle_of_a_batch():
    rs = np.random.RandomState(1)
    lens = [[5, 0, 250], [0, 0, 0, 0], [1]]
    trks, cands = zip(*[_tracklet(rs, len(n), i % 2, name=f't{i}') for i, n in enumerate(lens)])
    frames = [_frames(rs, t, n, 5, spread=(3, 3, 1)) for t, n in zip(trks, lens)]
    res, kept, _ = _check(_aug(), frames, list(trks), [list(c) for c in cands])
    assert len(kept[1]) == 0 and res['points'][1].shape == (0, 10) and len(kept[0]) > 0 and len(kept[2]) == 1
    assert res['pts_frame_inds'][1].shape == (0,) and res['counts'][1] == 0


@pytest.mark.parametrize('deco', [0, 1, 3, 5, 6, 8])
@pytest.mark.parametrize('cols', [3, 4, 5, 6, 8])
def test_every_pair_of_column_counts(cols, deco):
    """C + D from 3 to 16 columns: (5, 5) and (5, 6) take the kernels built for the shipped widths, the others the generic one"""
    rs = np.random.RandomState(16 * cols + deco)
    lens = [[40, 0, 300], [77]]
    trks, cands = zip(*[_tracklet(rs, len(n), 1, name=f't{i}') for i, n in enumerate(lens)])
    frames = [_frames(rs, t, n, cols) for t, n in zip(trks, lens)]
    aug = _aug(deco=deco)
    res, kept, _ = _check(aug, frames, list(trks), [list(c) for c in cands], _params(aug, trks, cols + deco))
    assert res['points'][0].shape[1] == cols + deco and len(kept[0]) > 10


@pytest.mark.parametrize('form', ['device frames', 'device rows', 'host rows', 'mixed'])
@pytest.mark.parametrize('cols,deco', [(5, 5), (8, 8), (3, 0)])
def test_host_and_device_inputs(cols, deco, form):
    rs = np.random.RandomState(cols)
    lens = [[40, 0, 300], [77, 2]]
    trks, cands = zip(*[_tracklet(rs, len(n), 0, name=f't{i}') for i, n in enumerate(lens)])
    frames = [_frames(rs, t, n, cols) for t, n in zip(trks, lens)]
    if form == 'device frames':
        give = [[torch.from_numpy(f).to(DEV) for f in fr] for fr in frames]
    elif form == 'device rows':
        give = [(torch.from_numpy(np.concatenate(fr)).to(DEV), n) for fr, n in zip(frames, lens)]
    elif form == 'host rows':
        give = [(np.concatenate(fr), np.array(n)) for fr, n in zip(frames, lens)]
    else:
        give = [[torch.from_numpy(f) for f in frames[0]], (torch.from_numpy(np.concatenate(frames[1])).to(DEV), lens[1])]
    aug = _aug(deco=deco, cut=dict(ratio=1.0, max_cut_ratio=0.9, min_length=2, max_length=150))
    _check(aug, frames, list(trks), None, _params(aug, trks, 5), give=give)


def test_over_limit_shapes_are_refused_by_name():
    import ctypes
    from sst_amd import _lib
    from sst_amd.tracklet_augment import MAX_FRAMES
    rs = np.random.RandomState(2)
    aug = _aug()
    trk, _ = _tracklet(rs, 2)
    for cols in (2, 9):
        with pytest.raises(NotImplementedError, match='point columns'):
            aug([[np.zeros((4, cols), F)] * 2], [copy.deepcopy(trk)], [[]])
    with pytest.raises(RuntimeError, match='use_dim=5'):
        _aug(use_dim=5)([[np.zeros((4, 4), F)] * 2], [copy.deepcopy(trk)], [[]])
    long_trk, _ = _tracklet(rs, MAX_FRAMES + 1, identity=True)
    with pytest.raises(NotImplementedError, match='SST_TRK_AUG_MAX_FRAMES'):
        _aug(train=False)([(np.zeros((3, 5), F), [3] + [0] * MAX_FRAMES)], [long_trk])
    with pytest.raises(RuntimeError, match='frames of points'):
        aug([[np.zeros((4, 5), F)]], [copy.deepcopy(trk)], [[]])
    # the entry point itself: nothing is launched
    a = _lib.TrackletAugmentArgs()
    counts = torch.zeros(1, dtype=torch.int32, device=DEV)
    a.counts, a.batch, a.cols, a.deco, a.n_total = counts.data_ptr(), 1, 5, 9, 0
    lib = _lib.load()
    assert lib.sst_tracklet_augment_points_f32(ctypes.byref(a), _lib.stream_ptr()) == _lib.SST_ERR_UNSUPPORTED
    a.deco, a.max_frames = 5, MAX_FRAMES + 1
    assert lib.sst_tracklet_augment_points_f32(ctypes.byref(a), _lib.stream_ptr()) == _lib.SST_ERR_UNSUPPORTED
    a.max_frames, a.n_total = 1, 10                                   # rows, but no buffers
    assert lib.sst_tracklet_augment_points_f32(ctypes.byref(a), _lib.stream_ptr()) == _lib.SST_ERR_ARG
    assert lib.sst_tracklet_augment_points_f32(None, _lib.stream_ptr()) == _lib.SST_ERR_ARG
    assert lib.sst_tracklet_augment_workspace_bytes(-1, 1) == 0 and lib.sst_tracklet_augment_workspace_bytes(10, 1) > 0


# ------------------------------------------------------------------------------------------------ range, identity
def test_range_bounds_are_strict_non_finite_rows_are_dropped_and_identity_keeps_the_bits():
    """a test pipeline under identity poses: the frame matrix is the unit matrix, the record scales by 1 and adds -0.0 - every
    surviving row leaves with the bits it came with; rows on each of the six bounds are dropped, one ulp inside they stay"""
    aug = _aug(train=False, shuffle=False, deco=5)
    r = np.array(RANGE, F)
    rows, expect = [], []
    for k in range(3):
        for bound, inward in ((r[k], F(np.inf)), (r[k + 3], F(-np.inf))):
            on = np.array([1.0, 2.0, 0.5, 0.0, 0.0], F)
            on[k] = bound
            inside = on.copy()
            inside[k] = np.nextafter(bound, inward)
            rows += [on, inside]
            expect += [False, True]
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            row = np.array([1.0, 2.0, 0.5, 0.0, 0.0], F)
            row[k] = bad
            rows.append(row)
            expect.append(False)
    pts = np.stack(rows)
    pts[:, 3] = np.arange(len(rows))
    rs = np.random.RandomState(3)
    trk, _ = _tracklet(rs, 3, identity=True)
    frames = [pts[:7], pts[7:7], pts[7:]]
    res, kept, per_sample = _check(aug, [frames], [trk])
    assert np.array_equal(kept[0], np.nonzero(expect)[0])
    assert np.array_equal(per_sample[0][0].numpy(), np.tile(np.eye(4, dtype=F), (3, 1, 1)))
    _bits(res['points'][0][:, :5], pts[kept[0]], 'identity')
    assert res['pts_frame_inds'][0].tolist() == [0 if i < 7 else 2 for i in kept[0]]


@pytest.mark.parametrize('flip_h,flip_v', list(itertools.product([False, True], repeat=2)))
def test_flip_combinations(flip_h, flip_v):
    rs = np.random.RandomState(4)
    trk, cands = _tracklet(rs, 6, 2)
    frames = _frames(rs, trk, [50, 0, 70, 3, 64, 100], 5)
    aug = _aug()
    res, kept, _ = _check(aug, [frames], [trk], [cands], _params(aug, [trk], 6, flip_h=flip_h, flip_v=flip_v))
    assert res['pcd_horizontal_flip'] == [flip_h] and res['pcd_vertical_flip'] == [flip_v] and len(kept[0]) > 20


# ------------------------------------------------------------------------------------------------ shuffle
def test_shuffle_is_a_reproducible_permutation():
    rs = np.random.RandomState(6)
    trk, _ = _tracklet(rs, 4)
    frames = _frames(rs, trk, [20, 0, 30, 14], 5, spread=(3, 3, 0.3))                     # all 64 rows inside the range
    aug = _aug()
    p = _params(aug, [trk], 7)
    shuffled, kept, _ = _check(aug, [frames], [copy.deepcopy(trk)], None, p)
    a, fa = shuffled['points'][0].cpu().numpy().copy(), shuffled['pts_frame_inds'][0].cpu().numpy().copy()
    again, _, _ = _check(aug, [frames], [copy.deepcopy(trk)], None, p)
    _bits(again['points'][0], a, 'same seed')
    _bits(again['pts_frame_inds'][0], fa, 'same seed')
    plain, kept_plain, _ = _check(_aug(shuffle=False), [frames], [copy.deepcopy(trk)], None, p)
    b, fb = plain['points'][0].cpu().numpy(), plain['pts_frame_inds'][0].cpu().numpy()
    assert len(kept[0]) == 64 and np.array_equal(kept_plain[0], np.arange(64)) and not np.array_equal(kept[0], kept_plain[0])
    assert np.array_equal(np.sort(kept[0]), kept_plain[0])
    assert np.array_equal(a, b[kept[0]]) and np.array_equal(fa, fb[kept[0]])             # a permutation of the unshuffled output
    assert fb.tolist() == [0] * 20 + [2] * 30 + [3] * 14
    p2 = copy.deepcopy(p)
    p2.seed[0] += np.uint64(2)
    _, kept2, _ = _check(aug, [frames], [copy.deepcopy(trk)], None, p2)
    assert not np.array_equal(kept2[0], kept[0]) and np.array_equal(np.sort(kept2[0]), np.arange(64))


def test_shuffle_orders_are_uniform():
    """one call, one seed, 2 400 one-frame tracklets of 4 in-range rows: each of the 24 orders occurs between 50 and 150 times
    (expected 100, standard deviation 9.8: the bound is 5 sigma), as DESIGN.md 3.26 tests it"""
    import sst_amd
    from sst_amd.tracklet_augment import TrackletParams
    batch = 2400
    aug = _aug(train=False, deco=0)
    pts = np.zeros((4, 4), F)
    pts[:, 0], pts[:, 3] = [1, 2, 3, 4], [0, 1, 2, 3]
    trks = []
    for i in range(batch):
        t = sst_amd.LiDARTracklet('seg', str(i), 0, True, torch.ones(1, 7), [T.TS0], [0.5])
        t.freeze()
        t.pose_list = [torch.eye(4)]
        trks.append(t)
    p = TrackletParams(batch)
    p.seed[:] = np.uint64(0x0123456789ABCDEF)
    res = aug([(pts, [4])] * batch, trks, None, p)
    assert res['offsets'] == list(range(0, 4 * batch + 1, 4))
    order = res['points_packed'][:, 3].cpu().numpy().astype(np.int64).reshape(batch, 4)
    assert (np.sort(order, 1) == np.arange(4)).all()
    for s in (0, 1, 1234, batch - 1):
        assert np.array_equal(order[s], np.argsort(R.shuffle_keys(p.seed[s], s, 4), kind='stable'))
    counts = np.bincount(order @ np.array([64, 16, 4, 1]), minlength=256)
    counts = counts[counts > 0]
    print('orders:', len(counts), 'min', counts.min(), 'max', counts.max())
    assert len(counts) == 24 and counts.min() >= 50 and counts.max() <= 150


# ------------------------------------------------------------------------------------------------ frame indices
def test_frame_indices_are_the_uploaded_values_also_after_a_cut():
    """TrackletCutting keeps the frame indices of before the cut: the kept frames' values start at `head`"""
    rs = np.random.RandomState(8)
    trk, cands = _tracklet(rs, 12, 1)
    frames = _frames(rs, trk, [3, 0, 5, 70, 1, 1, 0, 2, 64, 9, 4, 6], 5, spread=(3, 3, 1))
    aug = _aug(shuffle=False)
    p = _params(aug, [7], 1)                                          # the noise of the 7 frames that stay
    p.cut[0] = (3, 2)                                                 # a cut replayed by hand: head 3, tail 2
    res, kept, per_sample = _check(aug, [frames], [trk], [cands], p)
    assert per_sample[0][3] == (3, 7) and len(trk) == 7 and len(cands[0]) > 7           # the candidates are not cut
    lens = [70, 1, 1, 0, 2, 64, 9]
    assert res['pts_frame_inds'][0].tolist() == np.repeat(np.arange(3, 10), lens).tolist() and res['pts_frame_inds'][0].dtype == torch.int32
    assert res['counts'] == [sum(lens)]


# ------------------------------------------------------------------------------------------------ the golden of the host test
@pytest.mark.parametrize('matrices', ['the reference\'s', 'the library\'s'])
def test_golden_end_to_end_through_the_kernels(monkeypatch, matrices):
    """the four chains of tests/golden/tracklet_pipeline.npz as ONE batch.  With the reference's frame matrices handed to the
    host side: the surviving rows and their frame indices are the reference's, the coordinates and the boxes stay within the
    bars of tests/test_tracklet_augment_host.py.  With the library's own matrices (one batched product per sample), which the
    host test holds within max(4 x the reference's float32-vs-float64 gap, 1e-6) of the reference's largest element: that bar,
    applied to a row (|x| + |y| + |z| + 1), is added to the coordinates, and the surviving sets may differ only in rows whose
    reference coordinate lies within its tolerance of a range bound (the golden keeps 1e-3 m clear; the matrices of a pose
    10^4 m from the origin differ by up to 2e-3 m)."""
    import sst_amd.tracklet_augment as TA
    import test_tracklet_augment_host as H
    g = R.load_golden(GOLDEN)
    cases = H.cases(g)
    own = matrices == 'the library\'s'
    if not own:
        table = {}
        for r in cases:
            head, tail, _ = H.kept_frames(r)
            table[r['poses'][head:len(r['ts']) - tail].tobytes()] = r['mm']
            for c in r['cands']:
                table[c['poses'].tobytes()] = c['mm']
        monkeypatch.setattr(TA, 'frame_matrices', lambda center, poses: torch.as_tensor(table[np.stack([np.asarray(q, F) for q in poses]).tobytes()]))
    aug = _aug(deco=6, shuffle=False, cut=dict(ratio=0.0, max_length=150))
    trks, cands, p = [], [], TA.TrackletParams(len(cases))
    for i, r in enumerate(cases):
        t, c, q = H.golden_batch(r)
        trks.append(t)
        cands.append(c)
        for key in ('cut', 'center_noise', 'size_noise', 'yaw_noise'):
            getattr(p, key)[i] = getattr(q, key)[0]
        p.flip_h[i], p.flip_v[i], p.angle[i], p.scale[i], p.trans[i] = q.flip_h[0], q.flip_v[0], q.angle[0], q.scale[0], q.trans[0]
    res, kept, per_sample = _check(aug, [r['frames'] for r in cases], trks, cands, p)
    rng6 = np.asarray(RANGE, np.float64)
    for i, r in enumerate(cases):
        head, tail, frames = H.kept_frames(r)
        rows = np.concatenate(frames)
        of = np.repeat(np.arange(len(frames)), [len(f) for f in frames])
        mat_tol = (max(4 * float(r['gap_mm']), 1e-6) * np.abs(r['mm']).max() * (np.abs(rows[:, :3]).sum(1) + 1)) if own else np.zeros(len(rows))
        pose_tol = H.POSE_BAR_ULP * H.pose_unit(rows[:, :3], r['mm'][of]) + mat_tol[:, None]
        rot_tol = H.ROT_CEILING_ULP * H._ulp(np.abs(r['flip_points'][:, 0]) + np.abs(r['flip_points'][:, 1]))
        tol_xy = 1.05 * (pose_tol[:, :2].sum(1) + rot_tol) + H._ulp(r['scale_points'][:, :2]).max(1) + H._ulp(r['trans_points'][:, :2]).max(1)
        tol_z = 1.05 * pose_tol[:, 2] + H._ulp(r['scale_points'][:, 2]) + H._ulp(r['trans_points'][:, 2])
        ref_kept = np.nonzero(r['mask'])[0]
        if not own:
            assert np.array_equal(kept[i], ref_kept)
            assert np.array_equal(res['pts_frame_inds'][i].cpu().numpy(), r['final_frame_inds'])
        else:
            tol3 = np.stack([tol_xy, tol_xy, tol_z], 1)
            x = r['trans_points'].astype(np.float64)
            near = ((np.abs(x - rng6[None, :3]) <= tol3) | (np.abs(x - rng6[None, 3:]) <= tol3)).any(1)
            assert near[np.setxor1d(kept[i], ref_kept)].all()
        both = np.isin(kept[i], ref_kept)
        out = res['points'][i].cpu().numpy()[both]
        m = kept[i][both]
        assert len(m) >= len(ref_kept) - 5
        assert (np.abs(out[:, :2].astype(np.float64) - r['trans_points'][m][:, :2]) <= tol_xy[m][:, None]).all()
        assert (np.abs(out[:, 2].astype(np.float64) - r['trans_points'][m][:, 2]) <= tol_z[m]).all()
        assert np.array_equal(out[:, 3:5], rows[m][:, 3:5])
        deco = out[:, 5:]
        want = np.nan_to_num(r['deco'])[of][m]
        assert np.array_equal(deco[:, 1:], want[:, 1:])                                    # size, score, length: no matrix involved
        assert np.abs(deco[:, 0].astype(np.float64) - want[:, 0]).max() <= max(4 * float(r['gap_noise_boxes']), 1e-6) * np.abs(r['noise_boxes']).max()
        rel = lambda a, b: np.abs(a.astype(np.float64) - b).max() / np.abs(b).max()      # noqa: E731
        bar = max(4 * float(r['gap_trans_boxes']), 1e-6) + 16 * 2.0 ** -24                 # + the rotation, scale, translation roundings
        assert rel(trks[i].boxes.cpu().numpy(), r['trans_boxes']) <= bar
        assert np.array_equal(trks[i].boxes.cpu().numpy()[:, 3:6], r['trans_boxes'][:, 3:6])
        for c, lib_c in zip(r['cands'], cands[i]):
            assert rel(lib_c.boxes.cpu().numpy(), c['trans_boxes']) <= bar
        assert np.array_equal(trks[i].shared_pose.numpy(), r['shared_pose']) and trks[i].rot_angle == float(r['rot_angle_attr'])


# ------------------------------------------------------------------------------------------------ into the detector, steady state
def test_targets_and_one_training_step_take_the_output():
    """tracklet_targets reads the boxes where the call left them (one device buffer, no host copy), and a small TrackletDetector
    from the shipped model dictionary takes points, frame indices, tracklets and candidates as they come"""
    import sst_amd
    import test_gpu_tracklet_detector as D
    torch.manual_seed(3)
    det = sst_amd.build_detector(D.small_model()).to(DEV).train()
    points, frame_inds, trks, cand_lists = D.make_batch(11)
    frames = []
    for pts, fi, trk in zip(points, frame_inds, trks):
        order = torch.argsort(fi, stable=True)
        frames.append((pts[order][:, :5].contiguous().numpy(), np.bincount(fi.numpy(), minlength=len(trk))))
        trk.shared_pose = None
        for c in cand_lists[trks.index(trk)]:
            c.pose_list = [torch.eye(4) for _ in range(len(c))]
    aug = _aug(rng=D.RANGE)
    p = _params(aug, trks, 0, angle=0.05, scale=1.0, trans=0.0)
    res = aug(frames, trks, cand_lists, p)
    assert all(0 < q.shape[0] and q.shape[1] == 10 for q in res['points'])
    assert all(m.boxes.is_cuda for t, cl in zip(trks, cand_lists) for m in [t] + cl)
    targets = sst_amd.tracklet_targets(trks, cand_lists, dict(candidate_thresh=0.5, assigner=dict(object_centric=False, iou_thr=0.5),
                                                                cls_pos_thr=(0.8,), cls_neg_thr=(0.2,)), num_classes=1)
    assert targets['boxes'].is_cuda and torch.equal(targets['boxes'], torch.cat([t.boxes for t in trks]))
    assert torch.equal(targets['gts'], torch.cat([c.boxes for cl in cand_lists for c in cl])) and int(targets['counts'].sum()) > 0
    losses = det.forward_train(res['points'], [f.long() for f in res['pts_frame_inds']], None, trks, cand_lists)
    flat = [v for val in losses.values() for v in (val if isinstance(val, (list, tuple)) else [val])]
    assert flat and all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in flat) and float(losses['num_pos_rois']) > 0


@pytest.mark.parametrize('on_device', [False, True])
def test_later_calls_allocate_nothing_on_the_device(on_device):
    rs = np.random.RandomState(3)
    aug = _aug()
    allocs = []
    for it in range(3):
        lens = [[40, 0, 300, 9], [77, 2]]
        same = np.random.RandomState(5)                               # the same tracklets and candidates every time: one shape
        trks, cands = zip(*[_tracklet(same, len(n), 1 + i, name=f't{i}') for i, n in enumerate(lens)])
        frames = [(np.concatenate(_frames(rs, t, n, 5)), n) for t, n in zip(trks, lens)]
        if on_device:
            frames = [(torch.from_numpy(f).to(DEV), n) for f, n in frames]
        p = _params(aug, trks, it)
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()['allocation.all.allocated']
        res = aug(frames, list(trks), [list(c) for c in cands], p)
        torch.cuda.synchronize()
        allocs.append(torch.cuda.memory_stats()['allocation.all.allocated'] - before)
        assert res['points_packed'].shape[0] > 0
    assert allocs[0] > 0 and allocs[1:] == [0, 0]
