"""The CTRL test-time augmentation on the GPU (csrc/tracklet_tta.hip through sst_amd.tracklet_tta) against
tests/tracklet_tta_ref.py, the restatement tests/test_tracklet_tta_host.py pins to the reference's classes.

Views: everything is EQUAL bit for bit to the restatement - rows, their order, frame indices, counts, the boxes of every view.
Finish: the per-view boxes stay within max(4 x the golden's own float32-vs-float64 gap, 1e-6) of the reference's (the device's
sin / cos / atan2 and the stated order of the matrix product are not the CPU's); the merged outputs equal the fp64 numpy merge of
the kernel's OWN per-view outputs bit for bit.  Detector: aug_test equals K passes of B samples by hand bit for bit (one pass over
the K * B samples does not: the vendor GEMM of the box head's fp32 linears rounds in another order when the batch grows).
The shapes are the smallest at which the kernels can go wrong: samples of 0, 255, 256 and 257 rows (the classify workgroup),
tracklets of 1, 2 and 37 frames with empty frames, 1, 4 and 32 views."""
import copy
import os

import numpy as np
import pytest
import torch

import tracklet_ref as T
import tracklet_tta_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F = np.float32
RANGE = [-24.0, -24.0, -2.5, 24.0, 24.0, 3.0]
PROPS = {0: [], 5: ['yaw', 'size', 'score'], 6: ['yaw', 'size', 'score', 'length'], 8: ['size', 'yaw', 'size', 'score']}
ROTS8 = [0.0, 0.4, -0.4, 1.1, -1.1, 2.0, -2.0, 3.0]
MODES = ('max', 'weighted', 'iou_clamped_weighted')


def _pipeline(rots=0, flip=True, h=True, v=True, deco=5, rng=RANGE, shuffle=True):
    inner = [dict(type='TrackletGlobalRotScaleTrans', rot_range=[0, 0], scale_ratio_range=[1.0, 1.0], translation_std=[0, 0, 0]),
             dict(type='TrackletRandomFlip', flip_ratio_bev_horizontal=0.0, flip_ratio_bev_vertical=0.0)]
    if rng is not None:
        inner.append(dict(type='PointsRangeFilter', point_cloud_range=list(rng)))
    if shuffle:
        inner.append(dict(type='PointShuffle'))
    inner += [dict(type='TrackletFormatBundle', class_names=['Car']), dict(type='Collect3D', keys=['points', 'pts_frame_inds', 'tracklet'])]
    return [dict(type='LoadTrackletPoints', load_dim=6, use_dim=None, max_points=1024), dict(type='TrackletPoseTransform', concat=False),
            dict(type='PointDecoration', properties=PROPS[deco], concat=True),
            dict(type='MultiScaleFlipAug3D', img_scale=(1333, 800), pts_scale_ratio=1, pts_rots=rots, flip=flip, pcd_horizontal_flip=h,
                 pcd_vertical_flip=v, transforms=inner)]


def _plan(**kw):
    from sst_amd.tracklet_tta import TrackletTTA
    return TrackletTTA.from_pipeline(_pipeline(**kw))


def _pose(k, identity=False):
    m = np.eye(4, dtype=F)
    if not identity:
        a = 0.3 + 0.004 * k
        m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        m[:3, 3] = [1.0e4 + 1.1 * k, -2.0e4 + 0.4 * k, 30 + 0.01 * k]
    return m


def _tracklet(rs, n, identity=False, name='t'):
    import sst_amd
    boxes = T.track_boxes(np.random.default_rng(rs.randint(1 << 30)), n, 0)
    boxes[:, :2] *= 0.2
    ts = [T.TS0 + 100_000 * k for k in range(n)]
    trk = sst_amd.LiDARTracklet('seg', name, 0, True, torch.as_tensor(boxes.copy()), ts, rs.uniform(0.1, 0.9, n).astype(F).tolist())
    trk.freeze()
    trk.set_type(0, 'mmdet3d')
    trk.pose_list = [torch.as_tensor(_pose(k, identity)) for k in range(n)]
    return trk


def _frames(rs, trk, lens, cols, spread=(30.0, 30.0, 3.5)):
    out = []
    for k, m in enumerate(lens):
        p = np.zeros((m, cols), F)
        p[:, :3] = trk.boxes[k, :3].numpy() + rs.uniform(-1, 1, (m, 3)) * spread
        p[:, 3:] = rs.uniform(0, 1, (m, cols - 3))
        out.append(p)
    return out


def _bits(got, want, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape, f'{what}: shape {got.shape} vs {want.shape}'
    assert got.dtype == want.dtype, f'{what}: {got.dtype} vs {want.dtype}'
    view = {4: np.int32, 8: np.int64}[got.dtype.itemsize] if got.dtype.kind == 'f' else got.dtype
    assert np.array_equal(got.view(view), want.view(view)), f'{what}: not bit for bit'


def _check_views(plan, frames, trks, seeds):
    """one call against the restatement, view by view and sample by sample -> (the result, the kept input rows per (view, sample))"""
    from sst_amd.tracklet_augment import TrackletParams
    batch, K = len(trks), plan.n_views
    per_sample, boxes, ranges = plan.prepare_boxes(copy.deepcopy(trks), None, TrackletParams(batch))
    poses = [np.stack([np.asarray(p) for p in t.pose_list]) for t in trks]
    old_scores = np.array([float(s) for t in trks for s in t.score_list])
    res = plan(frames, trks, seeds=seeds)
    assert res['n_views'] == K and res['batch'] == batch and len(res['points']) == K * batch == len(res['counts'])
    kept = []
    for k, view in enumerate(plan.views):
        for i in range(batch):
            mm, deco, values, _, center = per_sample[i]
            want, fi, idx = R.view_sample(frames[i], mm.numpy(), deco.numpy(), values, view, k, plan.point_range, plan.shuffle, seeds[i], i)
            j = k * batch + i
            _bits(res['points'][j], want, f'points of view {k} sample {i}')
            _bits(res['pts_frame_inds'][j], fi, f'frame indices of view {k} sample {i}')
            assert res['counts'][j] == want.shape[0] == res['offsets'][j + 1] - res['offsets'][j]
            kept.append(idx)
        _bits(res['boxes_views'][k], R.view_boxes(boxes.numpy(), view), f'boxes of view {k}')
    _bits(res['old_boxes'], boxes.numpy(), 'old boxes')
    _bits(res['ego_mats'], np.concatenate([R.ego_matrices(p, p[len(p) // 2])[:, :3, :].reshape(-1, 12) for p in poses]), 'ego matrices')
    _bits(res['old_scores'], old_scores, 'old scores')
    _bits(res['roi_scores'], old_scores.astype(F), 'roi scores')
    assert res['row_sample'].tolist() == [i for i, t in enumerate(trks) for _ in range(len(t))]
    assert res['row_frame'].tolist() == [f for t in trks for f in range(len(t))]
    assert res['points_packed'].shape[0] == res['offsets'][-1] == sum(len(x) for x in kept)
    for i, trk in enumerate(trks):
        r0, r1 = res['box_ranges'][i]
        assert trk.boxes.data_ptr() == res['old_boxes'][r0:r1].data_ptr() and torch.equal(trk.shared_pose, per_sample[i][4])
    return res, kept


def _batch(rs, cols=5):
    """tracklets of 37 frames (empty frames among them), 1 frame of 257 rows, 2 frames of 255 + 1 = 256 rows, 2 empty frames
    (0 rows: it owns no workgroup) and 1 frame of 255 rows"""
    lens = [rs.randint(0, 20, 37).tolist(), [257], [255, 1], [0, 0], [255]]
    lens[0][0] = lens[0][5] = lens[0][36] = 0
    trks = [_tracklet(rs, len(n), name=f't{i}') for i, n in enumerate(lens)]
    return trks, [_frames(rs, t, n, cols) for t, n in zip(trks, lens)], lens


# ------------------------------------------------------------------------------------------------ views
@pytest.mark.parametrize('K', [1, 4, 32])
def test_views_equal_the_restatement_and_two_runs_are_bit_equal(K):
    rs = np.random.RandomState(K)
    plan = _plan(**{1: dict(rots=[0.3], flip=False), 4: dict(), 32: dict(rots=ROTS8)}[K])
    assert plan.n_views == K
    trks, frames, lens = _batch(rs)
    seeds = [int(s) | 1 for s in rs.randint(1, 1 << 62, len(trks))]
    res, kept = _check_views(plan, frames, copy.deepcopy(trks), seeds)
    first = (res['points_packed'].cpu().numpy().copy(), res['frame_inds_packed'].cpu().numpy().copy(), list(res['counts']),
             res['boxes_views'].cpu().numpy().copy())
    assert all(0 < len(kept[k * 5 + i]) < sum(lens[i]) for k in range(K) for i in (0, 1, 2, 4)) and all(len(kept[k * 5 + 3]) == 0 for k in range(K))
    if K > 1:                       # the views shuffle differently: the same rows survive views 0 and 1 of sample 4 in another order
        a, b = kept[4], kept[5 + 4]
        assert not np.array_equal(a, b)
    again = plan(frames, copy.deepcopy(trks), seeds=seeds)
    _bits(again['points_packed'], first[0], 'second run')
    _bits(again['frame_inds_packed'], first[1], 'second run')
    _bits(again['boxes_views'], first[3], 'second run')
    assert again['counts'] == first[2]


def test_a_view_that_the_range_empties():
    """x > 0.5 only: every row survives the views that do not mirror x and none survives the two that do"""
    rs = np.random.RandomState(7)
    plan = _plan(rng=[0.5, -24.0, -2.5, 24.0, 24.0, 3.0])
    trks = [_tracklet(rs, 3, identity=True, name='a'), _tracklet(rs, 2, identity=True, name='b')]
    frames = []
    for t, lens in zip(trks, ([40, 0, 260], [7, 64])):
        fr = _frames(rs, t, lens, 5, spread=(3, 3, 0.3))
        for f in fr:
            f[:, 0] = np.abs(f[:, 0]) + 1
        frames.append(fr)
    res, kept = _check_views(plan, frames, trks, [5, 9])
    assert res['counts'] == [300, 71, 0, 0, 300, 71, 0, 0]
    assert res['points'][2].shape == (0, 10) and res['pts_frame_inds'][3].shape == (0,)


@pytest.mark.parametrize('cols,deco', [(5, 8), (3, 0), (5, 6), (8, 8)])
def test_column_counts(cols, deco):
    """5 + 5 and 5 + 6 take the gather built for the shipped widths, the others the generic one; 8 decoration values is the limit"""
    rs = np.random.RandomState(16 * cols + deco)
    plan = _plan(deco=deco)
    trks = [_tracklet(rs, 3, name='a'), _tracklet(rs, 1, name='b')]
    frames = [_frames(rs, trks[0], [40, 0, 300], cols), _frames(rs, trks[1], [77], cols)]
    res, kept = _check_views(plan, frames, trks, [3, 4])
    assert res['points'][0].shape[1] == cols + deco and len(kept[0]) > 10


def test_integer_data_is_exact():
    """integer coordinates under identity poses, rotations by 0 and +- pi / 2 and every flip: bit for bit with the restatement in
    every view, and in the views with angle 0 the coordinates are the integers themselves, mirrored"""
    rs = np.random.RandomState(11)
    plan = _plan(rots=[0.0, np.pi / 2, -np.pi / 2], shuffle=False)
    assert plan.n_views == 12
    trk = _tracklet(rs, 2, identity=True)
    frames = [np.concatenate([rs.randint(-30, 31, (m, 2)), rs.randint(-2, 3, (m, 1)), rs.randint(0, 5, (m, 2))], 1).astype(F)
              for m in (130, 127)]
    res, kept = _check_views(plan, [frames], [trk], [1])
    rows = np.concatenate(frames)
    for k, (h, v, angle) in enumerate(plan.views):
        if angle == 0.0:
            want = rows[kept[k]][:, :3] * np.array([-1 if v else 1, -1 if h else 1, 1], F)
            assert np.array_equal(res['points'][k][:, :3].cpu().numpy(), want + F(0.0))
        else:
            got = res['points'][k][:, :3].cpu().numpy()
            sign = 1 if angle > 0 else -1           # (x, y) -> (y, -x) * sign, up to cos(float32(pi / 2)) = -4.4e-8
            want = np.stack([sign * rows[kept[k]][:, 1], -sign * rows[kept[k]][:, 0]], 1) * np.array([-1 if v else 1, -1 if h else 1], F)
            assert np.abs(got[:, :2] - want).max() <= 30 * 4.4e-8 + np.spacing(F(30.0)) / 2


def test_one_view_equals_the_test_pipeline():
    """K = 1, no flip, angle 0: what TrackletAugment makes of the shipped test_pipeline with the same seeds (view 0 keeps the
    sample's seed); the boxes too"""
    from sst_amd.tracklet_augment import TrackletAugment, TrackletParams
    from sst_amd.tracklet_tta import TrackletTTA
    fix = os.path.join(GOLDEN, 'configs', 'pipeline', 'ctrl')
    test_pipeline = eval(open(os.path.join(fix, 'ctrl_veh_24e.pipeline.py')).read())['test_pipeline']
    tta_pipeline = eval(open(os.path.join(fix, 'ctrl_veh_24e.tta_pipeline.py')).read())['tta_pipeline']
    tta_pipeline[-1].update(flip=False)
    plan, aug = TrackletTTA.from_pipeline(tta_pipeline), TrackletAugment.from_pipeline(test_pipeline)
    assert plan.n_views == 1
    rs = np.random.RandomState(13)
    trks, frames, _ = _batch(rs)
    p = TrackletParams(len(trks))
    p.seed[:] = [11, 12, 13, 14, 15]
    a_trks, b_trks = copy.deepcopy(trks), copy.deepcopy(trks)
    want = aug(frames, a_trks, None, p)
    got = plan(frames, b_trks, seeds=[11, 12, 13, 14, 15])
    assert got['counts'] == want['counts'] and sum(want['counts']) > 500
    _bits(got['points_packed'], want['points_packed'].cpu().numpy(), 'points')
    _bits(got['frame_inds_packed'], torch.cat(want['pts_frame_inds']).cpu().numpy(), 'frame indices')
    _bits(got['boxes_views'][0], want['boxes_packed'].cpu().numpy() + F(0.0), 'boxes')


def test_over_limit_calls_are_refused():
    import ctypes
    from sst_amd import _lib
    lib = _lib.load()
    counts = torch.zeros(4, dtype=torch.int32, device=DEV)
    a = _lib.TrackletTTAViewsArgs()
    a.counts, a.batch, a.cols, a.deco, a.n_total, a.n_views = counts.data_ptr(), 1, 5, 5, 0, 33
    assert lib.sst_tracklet_tta_views_f32(ctypes.byref(a), _lib.stream_ptr()) == _lib.SST_ERR_UNSUPPORTED
    a.n_views, a.n_total = 4, 10                                       # rows, but no buffers
    assert lib.sst_tracklet_tta_views_f32(ctypes.byref(a), _lib.stream_ptr()) == _lib.SST_ERR_ARG
    a.n_total = 0
    counts += 7
    assert lib.sst_tracklet_tta_views_f32(ctypes.byref(a), _lib.stream_ptr()) == 0 and counts.tolist() == [0, 0, 0, 0]
    with pytest.raises(NotImplementedError, match='point columns'):
        _plan()([[np.zeros((4, 9), F)]], [_tracklet(np.random.RandomState(0), 1)])


# ------------------------------------------------------------------------------------------------ finish
@pytest.fixture(scope='module')
def golden():
    g = R.load_golden(GOLDEN)
    return g, [R.golden_case(g, c) for c in range(int(g['n_cases']))]


def _finish(r, mode, thresh, return_views=True):
    from sst_amd.tracklet_tta import tta_finish
    dev = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x)).to(dt).to(DEV)        # noqa: E731
    mm = R.ego_matrices(r['poses'], r['shared_pose'])
    return tta_finish(dev(r['pred'], torch.float32), dev(r['pred_scores'], torch.float32), dev(r['valid'], torch.bool),
                      dev(r['pose_boxes'], torch.float32), dev(r['scores'], torch.float64), dev(mm[:, :3, :].reshape(-1, 12), torch.float32),
                      r['views'], mode, thresh, return_views=return_views), mm


def _device_iou(a, b):
    import sst_amd
    return sst_amd.aligned_iou_3d(torch.as_tensor(a).to(DEV).contiguous(), torch.as_tensor(b).to(DEV).contiguous()).cpu().numpy()


def test_per_view_boxes_within_the_reference_gap(golden):
    """against the reference's per-view boxes (and the restatement in the kernel's order): max(4 x the golden's float32-vs-
    float64 gap, 1e-6) relative to the largest element, the yaw compared on the circle; the scores are equal"""
    g, cases = golden
    for c, r in enumerate(cases):
        out, mm = _finish(r, 'weighted', 0.0)
        got = out['view_boxes'].cpu().numpy()
        want, scores = R.update_views(r['pred'], r['pred_scores'], r['valid'], r['pose_boxes'], r['scores'], mm, r['views'], einsum=False)
        _bits(out['view_scores'], scores, 'view scores')
        _bits(out['view_scores'], r['ego_scores'], 'view scores against the reference')
        assert np.array_equal(got[..., 3:6], r['ego'][..., 3:6])
        bar = T.bar(float(r['gap_ego']))
        for name, ref in (('reference', r['ego']), ('restatement', want)):
            d = got.astype(np.float64) - ref
            d[..., 6] = (d[..., 6] + np.pi) % (2 * np.pi) - np.pi
            err = np.abs(d).max() / np.abs(r['ego']).max()
            print(f'case {c} K {len(r["views"])} per-view boxes against the {name}: {err:.3e} (bar {bar:.3e})')
            assert err <= bar


@pytest.mark.parametrize('mode', MODES)
def test_merge_equals_the_fp64_merge_of_the_kernels_own_views(golden, mode):
    g, cases = golden
    thresh = float(g['iou_merge_thresh'])
    seen, clamped, ties, all_invalid = set(), 0, 0, 0
    for r in cases:
        K, n = r['pred_scores'].shape
        out, _ = _finish(r, mode, thresh)
        plain, _ = _finish(r, 'weighted', thresh)                       # the scores before the clamp
        vb, vs = out['view_boxes'].cpu().numpy(), plain['view_scores'].cpu().numpy()
        _bits(plain['view_boxes'], vb, 'the per-view boxes do not depend on the mode')
        boxes, scores, used = R.merge(vb, vs, mode, thresh, iou_fn=_device_iou)
        _bits(out['view_scores'], used, 'effective scores')
        got_b, got_s = out['merged_boxes'].cpu().numpy(), out['merged_scores'].cpu().numpy()
        assert np.array_equal(got_b, boxes, equal_nan=True) and np.array_equal(got_s, scores, equal_nan=True)
        assert got_b.dtype == np.float64 and got_s.dtype == np.float64 and got_b.shape == (n, 7)
        lean, _ = _finish(r, mode, thresh, return_views=False)          # the per-view boxes in the workspace
        _bits(lean['merged'], out['merged'].cpu().numpy(), 'workspace path')
        seen.add(K)
        all_invalid += int((~r['valid']).all(0).sum())
        if mode == 'iou_clamped_weighted' and K > 1:
            clamped += int((used[1:] == 0).all(0).sum())
        if mode == 'max' and K > 2 and n > 8:
            top = vs.max(0)
            tie = (vs[1] == top) & (vs[2] == top) & (vs[0] < top)
            ties += int(tie.sum())
            assert np.array_equal(got_b[tie], vb[1][tie].astype(np.float64))          # the first of two equal maxima
    assert {1, 2, 3, 4, 5, 32} <= seen and all_invalid >= 5 and 1 in [len(r['boxes']) for r in cases]
    assert clamped >= 4 or mode != 'iou_clamped_weighted'
    assert ties >= 4 or mode != 'max'


@pytest.mark.parametrize('mode', MODES)
def test_zero_and_nan_scores_follow_ieee(mode):
    """a row whose scores are all zero (0 / 0), one with a NaN score, one whose yaws are equal in every view (ties in the
    median's ranks) and one ordinary, K = 4 views that change nothing"""
    from sst_amd.tracklet_tta import tta_finish
    rs = np.random.RandomState(3)
    K, n = 4, 4
    views = [(False, False, 0.0)] * K
    base = T.track_boxes(np.random.default_rng(1), n, 0)
    pred = np.stack([T.jitter(np.random.default_rng(k), base, 0.2) for k in range(K)])
    scores = rs.uniform(0.1, 0.9, (K, n)).astype(F)
    scores[:, 0] = 0
    scores[2, 1] = np.nan
    pred[:, 2, 6] = 0.25
    eye = np.tile(np.eye(4, dtype=F)[:3].reshape(1, 12), (n, 1))
    dev = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x)).to(dt).to(DEV)        # noqa: E731
    out = tta_finish(dev(pred, torch.float32), dev(scores, torch.float32), dev(np.ones((K, n), bool), torch.bool), dev(base, torch.float32),
                     dev(np.full(n, 0.5), torch.float64), dev(eye, torch.float32), views, mode, 0.3)
    vb = out['view_boxes'].cpu().numpy()
    boxes, sc, used = R.merge(vb, scores.astype(np.float64), mode, 0.3, iou_fn=_device_iou)
    got_b, got_s = out['merged_boxes'].cpu().numpy(), out['merged_scores'].cpu().numpy()
    assert np.array_equal(got_b, boxes, equal_nan=True) and np.array_equal(got_s, sc, equal_nan=True)
    assert np.array_equal(out['view_scores'].cpu().numpy(), used, equal_nan=True)
    if mode != 'max':
        assert np.isnan(got_b[0, :6]).all() and np.isfinite(got_b[0, 6]) and got_s[0] == 0 and np.isnan(got_s[1])


# ------------------------------------------------------------------------------------------------ detector
def _raw_batch(seed, empty=None):
    """the batch of tests/test_gpu_tracklet_detector.py as the loader leaves it: per-frame rows of 5 columns, tracklets with
    (identity) poses and no shared pose.  ``empty``: a sample whose points lie outside the range"""
    import test_gpu_tracklet_detector as D
    points, frame_inds, trks, _ = D.make_batch(seed)
    frames = []
    for i, (pts, fi, trk) in enumerate(zip(points, frame_inds, trks)):
        order = torch.argsort(fi, stable=True)
        rows = pts[order][:, :5].contiguous().numpy().copy()
        if i == empty:
            rows[:, 0] += 100
        frames.append((rows, np.bincount(fi.numpy(), minlength=len(trk))))
        trk.shared_pose = None
    return frames, trks


@pytest.fixture(scope='module')
def detector():
    import sst_amd
    import test_gpu_tracklet_detector as D
    torch.manual_seed(3)
    return sst_amd.build_detector(D.small_model()).to(DEV).eval()


def test_aug_test_raises_without_the_attach_call(detector):
    import sst_amd
    assert type(detector) is sst_amd.TrackletDetector
    with pytest.raises(NotImplementedError, match='aug_test'):
        detector.aug_test(None, None, None, None)


@pytest.mark.parametrize('merge,empty', [('weighted', None), ('iou_clamped_weighted', 1), ('max', None)])
def test_aug_test_equals_per_view_passes_and_the_restated_finish(detector, merge, empty):
    """aug_forward against K passes of B samples through the same modules by hand (the segmentor's simple_test, tracklets2rois,
    _bbox_forward, roi_decode on each view's slice): decoded boxes, scores and valid masks bit for bit; then the restated
    inverse and update within the bar of the finish tests and the fp64 merge of the kernel's own per-view boxes bit for bit;
    aug_test leaves the tracklets as merge_augs leaves result_list[0]"""
    import sst_amd
    import test_gpu_tracklet_detector as D
    from sst_amd.tracklet_tta import attach_tracklet_tta
    det = attach_tracklet_tta(copy.deepcopy(detector), dict(merge=merge, iou_merge_thresh=0.5), _pipeline(rng=D.RANGE))
    assert type(det) is sst_amd.TrackletTTADetector and type(detector) is sst_amd.TrackletDetector
    frames, trks = _raw_batch(12, empty)
    seeds = [21, 22, 23]
    out = det.aug_forward(frames, copy.deepcopy(trks), seeds=seeds)
    v = out['views']
    K, B, n = v['n_views'], v['batch'], sum(len(t) for t in trks)
    assert K == 4 and B == 3 and out['decoded_boxes'].shape == (K, n, 7)
    if empty is not None:
        assert all(v['counts'][k * B + empty] == 0 for k in range(K))
    head = det.roi_head
    # the segmentor applies tanh to the views' rows in place (as the reference does to its points): the passes by hand take the
    # views of a second, bit-equal call
    v = det.tta(frames, copy.deepcopy(trks), seeds=seeds)
    with torch.no_grad():
        for k in range(K):
            pts = det.fake_points_for_empty_input([p.clone() for p in v['points'][k * B:(k + 1) * B]])
            inds = det.fake_points_for_empty_input([f.long() for f in v['pts_frame_inds'][k * B:(k + 1) * B]])
            view_trks = copy.deepcopy(trks)
            for t, (r0, r1) in zip(view_trks, v['box_ranges']):
                t.boxes, t.device = v['boxes_views'][k, r0:r1, :7], v['boxes_views'].device
            seg = det.segmentor.simple_test(pts, inds, None)
            rois, roi_frame_inds, cls_preds, labels_3d = head.tracklets2rois(view_trks)
            res = head._bbox_forward(seg['seg_points'][:, :3], seg['seg_feats'], seg['batch_idx'], seg['pts_frame_inds'], rois, cls_preds,
                                     roi_frame_inds)
            boxes, scores, _ = sst_amd.roi_head.roi_decode(rois, res['bbox_pred'].contiguous(), res['cls_score'].contiguous(), with_bev=False)
            assert torch.equal(out['decoded_boxes'][k], boxes), f'view {k}: aug_forward decodes other boxes than a pass by hand'
            assert torch.equal(out['decoded_scores'][k], scores.view(-1)) and torch.equal(out['valid'][k], res['valid_roi_mask'])
    assert bool(out['valid'].any()) and (empty is None or not bool(out['valid'].all()))
    # the single pass over the K * B samples: the same RoIs are valid; the boxes differ by the vendor GEMM's rounding order in the
    # box head's fp32 linears (measured 2e-6 of the largest element on this model) - a sanity bound, not a parity claim
    det.tta_single_pass = True
    single = det.aug_forward(frames, copy.deepcopy(trks), seeds=seeds)
    det.tta_single_pass = False
    assert torch.equal(single['valid'], out['valid'])
    gap = float((single['decoded_boxes'] - out['decoded_boxes']).abs().max() / out['decoded_boxes'].abs().max())
    print(f'single pass against per-view passes: {gap:.3e} of the largest element')
    assert gap <= 1e-4
    # the restated finish on the decoded boxes
    old_scores = np.array([float(s) for t in trks for s in t.score_list])
    mm = np.tile(np.eye(4, dtype=F), (n, 1, 1))
    want, ws = R.update_views(out['decoded_boxes'].cpu().numpy(), out['decoded_scores'].cpu().numpy(), out['valid'].cpu().numpy(),
                              v['old_boxes'].cpu().numpy(), old_scores, mm, det.tta.views, einsum=False)
    vb = out['view_boxes'].cpu().numpy()
    d = vb.astype(np.float64) - want
    d[..., 6] = (d[..., 6] + np.pi) % (2 * np.pi) - np.pi
    assert np.abs(d).max() / np.abs(want).max() <= T.bar(0.0)
    boxes, scores, used = R.merge(vb, ws, merge, 0.5, iou_fn=_device_iou)
    assert np.array_equal(out['merged_boxes'].cpu().numpy(), boxes, equal_nan=True)
    assert np.array_equal(out['merged_scores'].cpu().numpy(), scores, equal_nan=True)
    _bits(out['view_scores'], used, 'effective scores')
    # aug_test and forward_test: the tracklets as merge_augs leaves them
    for call in (lambda t: det.aug_test(frames, None, None, t, seeds=seeds), lambda t: det.forward_test(frames, None, tracklet=t, seeds=seeds),
                 lambda t: det(return_loss=False, points=frames, img_metas=None, tracklet=t, seeds=seeds)):
        mine = copy.deepcopy(trks)
        res = call(mine)
        assert len(res) == B and all(a is b for a, b in zip(res, mine))
        for t, (r0, r1) in zip(res, v['box_ranges']):
            assert t.boxes.dtype == torch.float64 and not t.boxes.is_cuda and t.pose_list is None and len(t) == r1 - r0
            assert np.array_equal(t.boxes.numpy(), boxes[r0:r1], equal_nan=True) and t.score_list == scores[r0:r1].tolist()


def test_one_view_equals_simple_test(detector):
    """K = 1 with merge 'max': the decoded boxes are those of simple_test on TrackletAugment's test pipeline; the tracklets' boxes
    agree within 1e-6 of the largest element (the finish kernel's sin / cos / atan2 against torch's), the scores are equal"""
    import test_gpu_tracklet_detector as D
    from sst_amd.tracklet_augment import TrackletAugment, TrackletParams
    from sst_amd.tracklet_tta import attach_tracklet_tta
    tta_pipeline = _pipeline(rng=D.RANGE, flip=False)
    det = attach_tracklet_tta(copy.deepcopy(detector), dict(merge='max'), tta_pipeline)
    frames, trks = _raw_batch(12)
    got = det.aug_test(frames, None, None, copy.deepcopy(trks), seeds=[1, 2, 3])
    aug = TrackletAugment.from_pipeline(tta_pipeline[:3] + tta_pipeline[3]['transforms'][2:])
    p = TrackletParams(3)
    p.seed[:] = [1, 2, 3]
    plain = copy.deepcopy(trks)
    res = aug(frames, plain, None, p)
    with torch.no_grad():
        want = detector.simple_test(res['points'], None, [f.long() for f in res['pts_frame_inds']], plain)
    for a, b in zip(got, want):
        wb = b.concated_boxes().cpu().numpy().astype(np.float64)
        d = a.boxes.numpy() - wb
        d[:, 6] = (d[:, 6] + np.pi) % (2 * np.pi) - np.pi
        assert np.abs(d).max() / np.abs(wb).max() <= T.bar(0.0)
        assert a.score_list == [float(s) for s in b.score_list] and a.pose_list is None and b.pose_list is None
