"""The CTRL test-time augmentation without a GPU: tests/tracklet_tta_ref.py against the reference's classes
(tests/golden/tracklet_tta.npz, written by tests/golden/make_tracklet_tta.py), the plan ``TrackletTTA.from_pipeline`` builds and
refuses, the three shipped ``tta_pipeline`` fixtures, the argument errors of the C entry points, and the refusals that stay."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

import tracklet_ref as T
import tracklet_tta_ref as R
from test_augment_host import ROT_BAR_ULP, _rot_err_ulp
from test_configs_build import REF

GOLDEN_DIR = os.path.join(ROOT, 'tests', 'golden')
PIPE_DIR = os.path.join(GOLDEN_DIR, 'configs', 'pipeline', 'ctrl')
NAMES = ('ctrl_veh_24e', 'ctrl_ped_24e', 'ctrl_cyc_12e')
MODES = ('max', 'weighted', 'iou_clamped_weighted')


@pytest.fixture(scope='module')
def golden():
    return R.load_golden(GOLDEN_DIR)


def cases(g):
    return [R.golden_case(g, c) for c in range(int(g['n_cases']))]


def tta_fixture(name):
    return eval(open(os.path.join(PIPE_DIR, name + '.tta_pipeline.py')).read())['tta_pipeline']


def pipeline_of(case, point_range=(-24.0, -24.0, -2.5, 24.0, 24.0, 3.0), **over):
    """a tta_pipeline with the MultiScaleFlipAug3D arguments of a golden case"""
    steps = copy.deepcopy(tta_fixture('ctrl_veh_24e'))
    tta = steps[-1]
    tta.update(pts_rots=case['rots'], flip=case['flip'], pcd_horizontal_flip=case['h'], pcd_vertical_flip=case['v'])
    tta['transforms'][2]['point_cloud_range'] = list(point_range)
    tta.update(over)
    return steps


# ------------------------------------------------------------------------------------------------ restatement vs golden
def test_view_order_is_the_reference_loop(golden):
    from sst_amd.tracklet_tta import TrackletTTA
    seen = set()
    for case, r in zip(R.GOLDEN_CASES, cases(golden)):
        views = R.enumerate_views(case['flip'], case['h'], case['v'], case['rots'])
        assert [(float(h), float(v), a) for h, v, a in views] == [tuple(row) for row in r['view_table'].tolist()]
        assert TrackletTTA.from_pipeline(pipeline_of(case)).views == views
        seen.add(len(views))
    assert {1, 2, 3, 4, 5, 20, 32} <= seen


def test_view_boxes_bit_for_bit(golden):
    """bit for bit in every view with angle 0 (all views of the shipped configs) and in every column but the rotated centre
    elsewhere: the reference rotates through a BLAS matrix product whose order and fusing are the library's, and the restated
    2 x 2 product stays within the bar tests/test_augment_host.py derives and asserts for it (ROT_BAR_ULP of |x| + |y|)"""
    exact = rotated = 0
    worst = 0.0
    for r in cases(golden):
        for k, view in enumerate(r['views']):
            got = R.view_boxes(r['pose_boxes'], view)
            assert np.array_equal(got[:, 2:], r['aug_boxes'][k][:, 2:]), k
            if view[2] == 0.0:
                assert np.array_equal(got, r['aug_boxes'][k]), k
                exact += 1
            else:
                worst = max(worst, _rot_err_ulp(got, r['aug_boxes'][k], r['pose_boxes']))
                rotated += 1
    print(f'view boxes: {exact} views bit for bit, {rotated} rotated views, worst centre error {worst} ulp (bar {ROT_BAR_ULP})')
    assert exact >= 4 + 4 + 2 + 1 + 1 + 4 + 4 and rotated >= 1 + 2 + 4 + 16 + 28 and worst <= ROT_BAR_ULP


def test_view_points_masks_and_frame_indices(golden):
    """the view transform alone is pinned on the reference's own points (a view with angle 0 and no flip is the input of every
    other view: the rotation by 0 is idempotent): bit for bit where the angle is 0, z bit for bit and x, y within ROT_BAR_ULP
    elsewhere; the whole chain from the raw points stays within the pose step's bar and keeps the
    reference's rows and frame indices"""
    import tracklet_augment_ref as A
    checked, worst = 0, 0.0
    for r in cases(golden):
        of = np.repeat(np.arange(len(r['frame_lens'])), r['frame_lens'])
        assert np.array_equal(r['frame_inds'], of)
        posed = A.pose_points(r['points'][:, :3], r['mm'][of][:, :3, :])
        at = 0
        for k, view in enumerate(r['views']):
            xyz = R.view_points(posed, view)
            mask = A.in_range_3d(xyz, golden['range'])
            assert np.array_equal(mask, r['masks'][k]), k
            assert np.array_equal(of[mask], r['final_frame_inds'][at:at + int(mask.sum())])
            at += int(mask.sum())
            if 'xyz' in r:
                err = np.abs(xyz.astype(np.float64) - r['xyz'][k]).max() / np.abs(r['xyz'][k]).max()
                assert err <= T.bar(float(r['gap_xyz'])), (k, err)
        assert at == len(r['final_frame_inds']) and np.array_equal(r['counts'], r['masks'].sum(1))
        if 'xyz' in r and (False, False, 0.0) in r['views']:
            base = r['xyz'][r['views'].index((False, False, 0.0))]
            for k, view in enumerate(r['views']):
                got = R.view_points(base, view)
                assert np.array_equal(got[:, 2], r['xyz'][k][:, 2])
                if view[2] == 0.0:
                    assert np.array_equal(got, r['xyz'][k]), k
                else:
                    worst = max(worst, _rot_err_ulp(got, r['xyz'][k], base))
                checked += 1
    print(f'view points: {checked} views against the reference, worst rotated error {worst} ulp (bar {ROT_BAR_ULP})')
    assert checked >= 4 + 4 + 2 + 3 + 5 and worst <= ROT_BAR_ULP


def test_per_view_ego_boxes(golden):
    """inverse_aug and update_from_prediction.  The scores and the sizes are equal; the centre and the yaw go through the
    rotation and shared2ego's einsum - matrix products whose order is the BLAS library's - and, off the valid RoIs, the
    reference's old box went through the augmentation and back while this library uses the un-augmented one:
    within max(4 x the reference's own float32-vs-float64 gap, 1e-6), in both orders the restatement offers (the reference's
    einsum, and the kernel's ((m0 x + m1 y) + m2 z) + m3)"""
    for r in cases(golden):
        mm = R.ego_matrices(r['poses'], r['shared_pose'])
        for einsum in (True, False):
            ego, scores = R.update_views(r['pred'], r['pred_scores'], r['valid'], r['pose_boxes'], r['scores'], mm, r['views'], einsum)
            assert np.array_equal(scores, r['ego_scores'])
            assert np.array_equal(ego[..., 3:6], r['ego'][..., 3:6])
            d = ego.astype(np.float64) - r['ego']
            d[..., 6] = (d[..., 6] + np.pi) % (2 * np.pi) - np.pi
            err = np.abs(d).max() / np.abs(r['ego']).max()
            assert err <= T.bar(float(r['gap_ego'])), (einsum, err)
        assert (~r['valid']).any() or len(r['boxes']) == 1


@pytest.mark.parametrize('mode', MODES)
def test_merge_bit_for_bit(golden, mode):
    thresh = float(golden['iou_merge_thresh'])
    clamped = 0
    for r in cases(golden):
        boxes, scores, used = R.merge(r['ego'], r['ego_scores'], mode, thresh, iou_fn=lambda a, b: T.aligned_iou(a, b).numpy())
        assert boxes.dtype == np.float64 and scores.dtype == np.float64
        assert np.array_equal(boxes, r[f'merged_{mode}_boxes'], equal_nan=True), mode
        assert np.array_equal(scores, r[f'merged_{mode}_scores'], equal_nan=True), mode
        if mode == 'iou_clamped_weighted' and len(r['views']) > 1:
            clamped += int((used[1:] == 0).all(0).sum())
    if mode == 'iou_clamped_weighted':
        assert clamped >= 4                                   # rows whose clamped scores are all zero except view 0's


def test_median_yaw_for_one_to_five_views(golden):
    """np.median in the yaw's own dtype: K = 1 .. 5 (an even K takes the float32 mean of the two middle values)"""
    seen = set()
    for r in cases(golden):
        K = len(r['views'])
        if K > 5:
            continue
        yaw = np.sort(r['ego'][..., 6], 0)
        want = yaw[K // 2] if K % 2 else ((yaw[K // 2 - 1] + yaw[K // 2]) / np.float32(2)).astype(np.float32)
        assert np.array_equal(want.astype(np.float64), r['merged_weighted_boxes'][:, 6])
        seen.add(K)
    assert seen == {1, 2, 3, 4, 5}


def test_golden_margins(golden):
    thresh = float(golden['iou_merge_thresh'])
    taken, total = golden['taken_out'].tolist()
    assert taken <= 0.05 * total
    rng6 = golden['range']
    for r in cases(golden):
        if 'xyz' in r:
            for k in range(3):
                assert (np.abs(r['xyz'][..., k].astype(np.float64) - rng6[k]) >= 1e-3).all()
                assert (np.abs(r['xyz'][..., k].astype(np.float64) - rng6[k + 3]) >= 1e-3).all()
        assert (np.abs(r['ious'][1:].astype(np.float64) - thresh) >= 1e-4).all()


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize('name', NAMES)
def test_shipped_tta_pipelines_parse_to_four_views(name):
    from sst_amd.tracklet_tta import TrackletTTA
    plan = TrackletTTA.from_pipeline(tta_fixture(name))
    assert plan.n_views == 4 and plan.views == [(False, False, 0.0), (False, True, 0.0), (True, False, 0.0), (True, True, 0.0)]
    assert plan.use_dim == 5 and plan.properties == ('yaw', 'size', 'score') and plan.shuffle and plan.point_range is not None
    rec = plan.view_records([7, 9])
    assert rec.shape == (8,) and rec['flip_h'].tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and rec['flip_v'].tolist() == [0, 0, 1, 1, 0, 0, 1, 1]
    assert (rec['rotate'] == 1).all() and (rec['scale'] == 1).all() and (rec['cos'] == 1).all() and (rec['sin'] == 0).all()
    assert not np.signbit(rec['trans']).any() and rec['seed'].tolist() == [7, 9] * 4


@pytest.mark.parametrize('name', NAMES)
def test_tta_fixture_equals_the_config_text(name):
    path = os.path.join(REF, 'configs', 'ctrl', name + '.py')
    if not os.path.exists(path):
        pytest.skip('the reference tree is not on this machine')
    from sst_amd.optim import resolve_config
    cfg = resolve_config(open(path).read(), os.path.dirname(path), path)
    assert cfg['tta_pipeline'] == tta_fixture(name)


def _tta(**over):
    steps = copy.deepcopy(tta_fixture('ctrl_veh_24e'))
    steps[-1].update(over)
    return steps


def _inner(index, **over):
    steps = copy.deepcopy(tta_fixture('ctrl_veh_24e'))
    steps[-1]['transforms'][index].update(over)
    return steps


def _reordered():
    steps = copy.deepcopy(tta_fixture('ctrl_veh_24e'))
    t = steps[-1]['transforms']
    t[0], t[1] = t[1], t[0]
    return steps


@pytest.mark.parametrize('steps,word', [
    (_tta(pts_scale_ratio=[1, 1.1]), 'more than one scale'),
    (_tta(pts_scale_ratio=0.9), 'a scale that is not 1'),
    (_tta(flip_direction=['horizontal', 'vertical']), 'flip_direction'),
    (_inner(0, translation_std=[0, 0, 0.2]), 'translation_std'),
    (_inner(0, rot_range=[-0.1, 0.1]), 'rot_range'),
    (_inner(0, scale_ratio_range=[0.95, 1.05]), 'scale_ratio_range'),
    (_inner(0, shift_height=True), 'shift_height=True'),
    (_tta(pts_rots=[0.1 * i for i in range(9)]), 'SST_TRK_TTA_MAX_VIEWS'),
    (_reordered(), 'TrackletGlobalRotScaleTrans inside MultiScaleFlipAug3D'),
    (_tta(transforms=[dict(type='GlobalRotScaleTrans')]), 'GlobalRotScaleTrans inside MultiScaleFlipAug3D'),
    (_tta(transforms=tta_fixture('ctrl_veh_24e')[-1]['transforms'][1:]), 'without TrackletGlobalRotScaleTrans'),
    (_tta(transforms=tta_fixture('ctrl_veh_24e')[-1]['transforms'][:1]), 'without TrackletRandomFlip'),
    (tta_fixture('ctrl_veh_24e') + [tta_fixture('ctrl_veh_24e')[-1]], 'MultiScaleFlipAug3D'),
    (tta_fixture('ctrl_veh_24e')[:3], 'without MultiScaleFlipAug3D'),
    ([tta_fixture('ctrl_veh_24e')[0]] + tta_fixture('ctrl_veh_24e')[2:], 'without TrackletPoseTransform'),
    (tta_fixture('ctrl_veh_24e')[:1] + [dict(type='TrackletCutting')] + tta_fixture('ctrl_veh_24e')[1:], 'TrackletCutting'),
    (tta_fixture('ctrl_veh_24e')[:3] + [dict(type='TrackletRandomFlip')] + tta_fixture('ctrl_veh_24e')[3:], 'TrackletRandomFlip'),
    (tta_fixture('ctrl_veh_24e')[:1] + [dict(type='TrackletPoseTransform', centering=True)] + tta_fixture('ctrl_veh_24e')[2:], 'centering=True'),
    (tta_fixture('ctrl_veh_24e')[:2] + [dict(type='PointDecoration', properties=['center_offset'])] + tta_fixture('ctrl_veh_24e')[3:],
     'center_offset'),
])
def test_refusals_name_the_reason(steps, word):
    from sst_amd.tracklet_tta import TrackletTTA
    with pytest.raises(NotImplementedError, match=word):
        TrackletTTA.from_pipeline(steps)


def test_the_widest_plan_is_accepted():
    from sst_amd.tracklet_tta import MAX_VIEWS, TrackletTTA
    plan = TrackletTTA.from_pipeline(_tta(pts_rots=[0.1 * i for i in range(8)], img_scale=[(1, 1), (2, 2)]))
    assert plan.n_views == MAX_VIEWS == 32
    commented = TrackletTTA.from_pipeline(_tta(pts_rots=R.ROTS5))            # the configs' commented pts_rots, times double flip
    assert commented.n_views == 20


def test_attach_checks_its_arguments():
    import sst_amd
    from sst_amd.tracklet_tta import attach_tracklet_tta
    with pytest.raises(TypeError):
        attach_tracklet_tta(torch.nn.Linear(2, 2), dict(merge='max'), tta_fixture('ctrl_veh_24e'))
    model = eval(open(os.path.join(GOLDEN_DIR, 'configs', 'ctrl', 'ctrl_veh_24e.model.py')).read())
    det = sst_amd.build_detector(model)
    with pytest.raises(NotImplementedError, match='merge'):
        attach_tracklet_tta(det, dict(merge='mean'), tta_fixture('ctrl_veh_24e'))
    with pytest.raises(KeyError, match='iou_merge_thresh'):
        attach_tracklet_tta(det, dict(merge='iou_clamped_weighted'), tta_fixture('ctrl_veh_24e'))
    assert type(det) is sst_amd.TrackletDetector
    with pytest.raises(NotImplementedError, match='aug_test'):
        det.aug_test(None)
    out = attach_tracklet_tta(det, dict(merge='weighted'), tta_fixture('ctrl_veh_24e'))
    assert out is det and type(det) is sst_amd.TrackletTTADetector and det.tta.n_views == 4 and det.tta_cfg == dict(merge='weighted')
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no CPU path'):
            det.aug_test([[np.zeros((1, 5), np.float32)]], None, None, [None])


# ------------------------------------------------------------------------------------------------ what stays refused
def test_existing_refusals_remain():
    import sst_amd
    from sst_amd.tracklet_augment import TrackletAugment
    for name in NAMES:
        with pytest.raises(NotImplementedError, match='MultiScaleFlipAug3D'):
            TrackletAugment.from_pipeline(tta_fixture(name))
    model = eval(open(os.path.join(GOLDEN_DIR, 'configs', 'ctrl', 'ctrl_veh_24e.model.py')).read())
    bad = copy.deepcopy(model)
    bad['test_cfg']['tta'] = dict(merge='weighted')
    with pytest.raises(NotImplementedError, match='tta'):
        sst_amd.build_detector(bad)
    head = copy.deepcopy(model['roi_head'])
    with pytest.raises(NotImplementedError, match='tta'):
        sst_amd.build_head(dict(head, train_cfg=copy.deepcopy(model['train_cfg']), test_cfg=dict(model['test_cfg'], tta=dict(merge='max'))))
    with pytest.raises(NotImplementedError, match='aug_test'):
        sst_amd.TrackletDetector.aug_test(None)
    with pytest.raises(NotImplementedError, match='aug_test'):
        sst_amd.TrackletSegmentor.aug_test(None)
    with pytest.raises(NotImplementedError, match='merge_augs'):
        sst_amd.LiDARTracklet('seg', 'a', 1, True).merge_augs()


# ------------------------------------------------------------------------------------------------ the C entry points
def test_argument_errors_launch_nothing():
    from sst_amd import _lib
    lib = _lib.load()
    ARG, UNS = _lib.SST_ERR_ARG, _lib.SST_ERR_UNSUPPORTED
    assert lib.sst_tracklet_tta_views_f32(None, None) == ARG
    assert lib.sst_tracklet_tta_boxes_f32(None, None) == ARG
    assert lib.sst_tracklet_tta_finish(None, None) == ARG
    one = ctypes.c_void_p(16)           # a non-NULL, aligned address that is never read: every case below returns first

    def views(**kw):
        a = _lib.TrackletTTAViewsArgs()
        a.batch, a.cols, a.deco, a.n_views, a.n_total, a.counts = 1, 5, 5, 4, 0, one
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.sst_tracklet_tta_views_f32(ctypes.byref(a), None)

    assert views(cols=2) == UNS and views(cols=9) == UNS and views(deco=9) == UNS and views(deco=-1) == UNS
    assert views(n_views=33) == UNS and views(max_frames=2049) == UNS
    assert views(n_views=0) == ARG and views(batch=0) == ARG and views(n_total=-1) == ARG and views(counts=None) == ARG
    assert views(n_total=2 ** 30, n_views=4) == UNS
    assert views(n_total=10) == ARG                            # rows, and no pointer to them
    assert views(n_total=10, points=one, frame_rows=one, sample_frames=one, block_offsets=one, frames=one, frame_values=one,
                 params=one, out=one, out_frame_inds=one, workspace=one, n_blocks=1, n_frames=1, workspace_bytes=8) == ARG
    assert views(n_total=10, points=ctypes.c_void_p(20), frame_rows=one, sample_frames=one, block_offsets=one, frames=one,
                 frame_values=one, params=one, out=one, out_frame_inds=one, workspace=one, n_blocks=1, n_frames=1,
                 workspace_bytes=1 << 30) == ARG                 # a misaligned buffer
    assert lib.sst_tracklet_tta_views_workspace_bytes(1000, 2, 4, 10) > 0
    assert lib.sst_tracklet_tta_views_workspace_bytes(1000, 2, 33, 10) == 0 == lib.sst_tracklet_tta_views_workspace_bytes(-1, 2, 4, 10)
    assert lib.sst_tracklet_tta_views_workspace_bytes(1000, 2, 4, 2) == 0 == lib.sst_tracklet_tta_views_workspace_bytes(2 ** 30, 2, 4, 10)

    def boxes(**kw):
        b = _lib.TrackletTTABoxArgs()
        b.batch, b.cols, b.n_boxes, b.n_views, b.box_offsets, b.params = 1, 7, 0, 4, one, one
        for k, v in kw.items():
            setattr(b, k, v)
        return lib.sst_tracklet_tta_boxes_f32(ctypes.byref(b), None)

    assert boxes() == 0 and boxes(cols=8) == UNS and boxes(n_views=33) == UNS and boxes(n_views=0) == ARG and boxes(batch=0) == ARG
    assert boxes(n_boxes=-1) == ARG and boxes(params=None) == ARG and boxes(box_offsets=None) == ARG and boxes(n_boxes=3) == ARG

    def finish(**kw):
        a = _lib.TrackletTTAFinishArgs()
        a.n_rows, a.n_views, a.mode = 0, 4, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.sst_tracklet_tta_finish(ctypes.byref(a), None)

    assert finish() == 0 and finish(n_views=33) == UNS and finish(mode=3) == UNS and finish(mode=-1) == UNS
    assert finish(n_views=0) == ARG and finish(n_rows=-1) == ARG and finish(n_rows=5) == ARG
    full = dict(n_rows=5, boxes=one, scores=one, valid=one, old_boxes=one, old_scores=one, mats=one, merged_boxes=one, merged_scores=one)
    assert finish(**full) == ARG                                               # neither the per-view outputs nor a workspace
    assert finish(view_boxes=one, **full) == ARG                               # both or neither
    assert finish(workspace=one, workspace_bytes=8, **full) == ARG             # too small
    assert lib.sst_tracklet_tta_finish_workspace_bytes(5, 4) >= 5 * 4 * (8 + 28)
    assert lib.sst_tracklet_tta_finish_workspace_bytes(5, 33) == 0 == lib.sst_tracklet_tta_finish_workspace_bytes(-1, 4)
