"""The training augmentation on the host (no GPU): tests/augment_ref.py, the float32 restatement the kernels are held to, against
the reference's own classes.  The reference's arrays after every stage are in tests/golden/augment_golden*.npz, written by
tools/make_augment_golden.py from the reference's source text (ObjectSample, RandomFlip3D, GlobalRotScaleTrans, PointsRangeFilter,
ObjectRangeFilter, LiDARInstance3DBoxes, LiDARPoints, box_np_ops.points_in_rbbox); the generator takes out every input whose
reference output lies within 1e-3 m of a range bound and asserts that none is left, so no comparison below can hide a decision
that fell the other way."""
import ast
import glob
import os

import numpy as np
import pytest

import augment_ref as R
from conftest import ROOT

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
PIPELINES = sorted(glob.glob(os.path.join(GOLDEN, 'configs', 'pipeline', '*.pipeline.py')))
RUNS = [(fh, fv, si) for fh in (0, 1) for fv in (0, 1) for si in (0, 1)]
F = np.float32

# The rotation: x' = x c + y s written out against torch's `@` on [N, 3] x [3, 3].  Each side rounds two products and one sum
# (the third product is an exact zero): at most 1.5 ulp of |x| + |y| per side, 3 in all, so the derived ceiling is 4 ulp of
# |x| + |y|.  Measured on the golden inputs (8 runs, about 2 200 points and 18 boxes each): 1.0 ulp.  Asserted: twice that.
ROT_MEASURED_ULP = 1.0
ROT_BAR_ULP = min(2 * ROT_MEASURED_ULP, 4.0)


@pytest.fixture(scope='module')
def golden():
    return R.load_golden(GOLDEN)


def _ulp(v):
    return np.spacing(np.abs(v).astype(F)).astype(np.float64)


def _rot_err_ulp(ours, ref, before):
    unit = _ulp(np.abs(before[:, 0]) + np.abs(before[:, 1]))
    return float((np.abs(ours[:, :2].astype(np.float64) - ref[:, :2]) / unit[:, None]).max())


def test_stage_by_stage_against_the_reference_classes(golden):
    """every stage fed the reference's own previous-stage output: flips, scale, translation, both range masks, limit_yaw and
    every box column but the rotated centre are bit-equal; the rotation stays within ROT_BAR_ULP (measured maximum 1.0 ulp of
    |x| + |y|, points and box centres alike; derived ceiling 4)"""
    worst = 0.0
    for fh, fv, si in RUNS:
        r = R.golden_run(golden, fh, fv, si)
        rec = r['rec']
        assert np.array_equal(R.flip_points(r['s0_points'][:, :3], fh, fv), r['s1_points'])
        rot = R.rotate_points(r['s1_points'], rec['cos'], rec['sin'])
        assert np.array_equal(rot[:, 2], r['s2_points'][:, 2])
        worst = max(worst, _rot_err_ulp(rot, r['s2_points'], r['s1_points']))
        assert np.array_equal(R.scale_points(r['s2_points'], rec['scale']), r['s3_points'])
        assert np.array_equal(R.translate_points(r['s3_points'], rec['trans']), r['s4_points'])
        assert np.array_equal(R.in_range_3d(r['s4_points'], rec['range']), r['point_mask'])

        assert np.array_equal(R.flip_boxes(r['s0_boxes'], fh, fv), r['s1_boxes'])
        rot = R.rotate_boxes(r['s1_boxes'], rec['cos'], rec['sin'], rec['angle'])
        assert np.array_equal(rot[:, 2:], r['s2_boxes'][:, 2:])                  # yaw + angle included
        worst = max(worst, _rot_err_ulp(rot, r['s2_boxes'], r['s1_boxes']))
        assert np.array_equal(R.scale_boxes(r['s2_boxes'], rec['scale']), r['s3_boxes'])
        assert np.array_equal(R.translate_boxes(r['s3_boxes'], rec['trans']), r['s4_boxes'])
        assert np.array_equal(R.in_range_bev(r['s4_boxes'], rec['range']), r['box_mask'])
        assert np.array_equal(R.limit_yaw(r['s4_boxes'][r['box_mask']]), r['s5_boxes'])
    print(f'rotation: worst error {worst} ulp of |x| + |y| (bar {ROT_BAR_ULP})')
    assert worst <= ROT_BAR_ULP


def test_points_in_rbbox_through_the_restated_planes(golden):
    """random rotated float32 boxes (no reference sgn within 1e-4 of 0) and dyadic axis-aligned boxes with points exactly on
    faces, edges and corners: the masks equal the reference function's; on the dyadic data both sides are exact and sgn == 0
    counts as outside.  The planes themselves are bit-equal to surface_equ_3d's, and the package's to the restatement's."""
    from sst_amd.augment import box_planes
    planes = R.box_planes(golden['pib_boxes'])
    assert np.array_equal(planes[..., :3], golden['pib_normal']) and np.array_equal(planes[..., 3], golden['pib_d'])
    assert np.array_equal(box_planes(golden['pib_boxes']), planes)
    assert np.array_equal(R.points_in_planes(golden['pib_points'], planes), golden['pib_mask'])
    dy = R.box_planes(golden['dyadic_boxes'])
    assert np.array_equal(box_planes(golden['dyadic_boxes']), dy)
    pts = golden['dyadic_points']
    assert np.array_equal(R.points_in_planes(pts, dy), golden['dyadic_mask'])
    sgn = ((pts[:, None, None, 0] * dy[None, ..., 0] + pts[:, None, None, 1] * dy[None, ..., 1])
           + pts[:, None, None, 2] * dy[None, ..., 2]) + dy[None, ..., 3]
    on_face = (sgn == 0).any(-1) & (sgn <= 0).all(-1)            # on the closed box, touching a face
    assert on_face.sum() > 50 and not golden['dyadic_mask'][on_face].any()


def test_end_to_end_against_the_reference_chain(golden):
    """2 samples x the 4 flip combinations, C = 5, 12 ground-truth + 6 pasted boxes, |angle| <= pi / 4, translation_std 0.2:
    the kept points are the reference's as input rows (in its order), the kept boxes and labels are the reference's, and the
    coordinates stay within the rotation bar propagated through the scale (factor <= 1.05, one rounding on each side) and the
    translation (one rounding on each side): 1.05 * bar * ulp(|x| + |y|) + ulp(scaled) + ulp(translated); z, the other
    columns and every box column beyond the centre are bit-equal"""
    for fh, fv, si in RUNS:
        r = R.golden_run(golden, fh, fv, si)
        rec = r['rec']
        rows = np.concatenate([r['pasted_points'], r['in_points']])
        out, idx = R.augment_points(rows, r['pasted_points'].shape[0], R.box_planes(r['pasted']), rec, si)
        assert np.array_equal(idx, r['s0_rows'][r['point_mask']])
        want = np.concatenate([r['s4_points'], r['s0_points'][:, 3:]], 1)[r['point_mask']]
        tol = (1.05 * ROT_BAR_ULP * _ulp(np.abs(r['s1_points'][:, 0]) + np.abs(r['s1_points'][:, 1])) + _ulp(r['s3_points'][:, :2]).max(1)
               + _ulp(r['s4_points'][:, :2]).max(1))[r['point_mask']]
        assert (np.abs(out[:, :2].astype(np.float64) - want[:, :2]) <= tol[:, None]).all()
        assert np.array_equal(out[:, 2:], want[:, 2:])

        boxes, keep = R.transform_boxes(r['s0_boxes'], rec)
        assert np.array_equal(keep, r['box_mask'])
        assert np.array_equal(r['s0_labels'][keep], r['s5_labels'])
        tol = (1.05 * ROT_BAR_ULP * _ulp(np.abs(r['s1_boxes'][:, 0]) + np.abs(r['s1_boxes'][:, 1])) + _ulp(r['s3_boxes'][:, :2]).max(1)
               + _ulp(r['s4_boxes'][:, :2]).max(1))[keep]
        assert (np.abs(boxes[:, :2].astype(np.float64) - r['s5_boxes'][:, :2]) <= tol[:, None]).all()
        assert np.array_equal(boxes[:, 2:], r['s5_boxes'][:, 2:])


TRAIN = [dict(type='LoadPointsFromFile', coord_type='LIDAR', load_dim=6, use_dim=5),
         dict(type='ObjectSample', db_sampler=dict()),
         dict(type='RandomFlip3D', sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
         dict(type='GlobalRotScaleTrans', rot_range=[-0.78539816, 0.78539816], scale_ratio_range=[0.95, 1.05],
              translation_std=[0.5, 0.5, 0.2]),
         dict(type='PointsRangeFilter', point_cloud_range=[-74.88, -74.88, -2, 74.88, 74.88, 4]),
         dict(type='ObjectRangeFilter', point_cloud_range=[-74.88, -74.88, -2, 74.88, 74.88, 4]),
         dict(type='PointShuffle'), dict(type='DefaultFormatBundle3D', class_names=['Car']), dict(type='Collect3D', keys=['points'])]


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_draw_params_follows_the_reference_draws(golden, seed):
    """np.random.seed(k), a batch of 2: the flips, the rotation (as the cosine and sine of rot_mat_T and as the angle rounded to
    float32), pcd_scale_factor and pcd_trans equal what the reference's RandomFlip3D and GlobalRotScaleTrans,
    run from source sample after sample under the same seed, recorded"""
    from sst_amd.augment import TrainAugment
    aug = TrainAugment.from_pipeline(TRAIN)
    np.random.seed(seed)
    p = aug.draw_params(2)
    rec = p.records(np.ones(2, bool), aug.point_range, aug.shuffle)
    want = golden[f'draw_seed{seed}']
    assert np.array_equal(p.flip_h.astype(np.float64), want[:, 0]) and np.array_equal(p.flip_v.astype(np.float64), want[:, 1])
    assert np.array_equal(rec['cos'].astype(np.float64), want[:, 2]) and np.array_equal(rec['sin'].astype(np.float64), want[:, 3])
    assert np.array_equal(p.scale, want[:, 4]) and np.array_equal(p.trans, want[:, 5:8])
    assert np.array_equal(rec['angle'].astype(np.float64), want[:, 8])
    assert np.array_equal(rec['scale'], want[:, 4].astype(F)) and np.array_equal(rec['trans'], want[:, 5:8].astype(F))
    assert len(set(int(s) for s in p.seed)) == 2
    rs = np.random.RandomState(seed)                                   # a RandomState draws the same
    q = aug.draw_params(2, rs)
    assert np.array_equal(q.angle, p.angle) and np.array_equal(q.seed, p.seed)


def test_pipeline_fixtures_exist():
    assert len(PIPELINES) >= 8


@pytest.mark.parametrize('path', PIPELINES, ids=[os.path.basename(p) for p in PIPELINES])
def test_every_shipped_pipeline_builds(path):
    from sst_amd.augment import TrainAugment
    cfg = ast.literal_eval(open(path).read())
    train = TrainAugment.from_pipeline(cfg['train_pipeline'])
    assert train.object_sample and train.shuffle and train.flip == (0.5, 0.5) and train.rst is not None
    assert train.point_range is not None and np.array_equal(train.point_range, train.box_range)
    test = TrainAugment.from_pipeline(cfg['test_pipeline'])
    assert test.flip == 'off' and test.fixed_scale == 1.0 and not test.shuffle and test.box_range is None
    assert np.array_equal(test.point_range, train.point_range)
    p = test.draw_params(3)                                           # rotation 0, scale 1, no translation: the range filter alone
    assert not p.flip_h.any() and not p.flip_v.any() and not p.angle.any() and (p.scale == 1).all() and not p.trans.any()
    if 'nusc' in path:
        assert train.norm == ([3], [0.0], [255.0]) or train.norm is None


@pytest.mark.parametrize('step,name', [
    (dict(type='ObjectNoise'), 'ObjectNoise'), (dict(type='RandomJitterPoints'), 'RandomJitterPoints'),
    (dict(type='BackgroundPointsFilter', bbox_enlarge_range=(0.5, 2.0, 0.5)), 'BackgroundPointsFilter'),
    (dict(type='RandomPointDrop', drop_ratio=0.1), 'RandomPointDrop'),
    (dict(type='RandomFlip3D', sync_2d=True), 'sync_2d=True'), (dict(type='RandomFlip3D'), 'sync_2d=True'),
    (dict(type='GlobalRotScaleTrans', shift_height=True), 'shift_height=True'),
    (dict(type='ObjectSample', db_sampler=dict(), sample_2d=True), 'sample_2d=True'),
    (dict(type='TrackletRandomFlip'), 'TrackletRandomFlip'), (dict(type='TrackletGlobalRotScaleTrans'), 'TrackletGlobalRotScaleTrans'),
    (dict(type='IndoorPointSample', num_points=1000), 'IndoorPointSample'),
    (dict(type='MultiScaleFlipAug3D', flip=True, transforms=[]), 'MultiScaleFlipAug3D(flip=True)'),
    (dict(type='MultiScaleFlipAug3D', transforms=[dict(type='ObjectNoise')]), 'ObjectNoise')])
def test_refused_transforms_are_named(step, name):
    from sst_amd.augment import TrainAugment
    with pytest.raises(NotImplementedError, match=name.replace('(', r'\(').replace(')', r'\)')):
        TrainAugment.from_pipeline([dict(type='LoadPointsFromFile'), step])


def test_steps_out_of_kernel_order_are_refused():
    from sst_amd.augment import TrainAugment
    with pytest.raises(NotImplementedError, match='GlobalRotScaleTrans'):
        TrainAugment.from_pipeline([dict(type='PointsRangeFilter', point_cloud_range=[-1, -1, -1, 1, 1, 1]),
                                    dict(type='GlobalRotScaleTrans')])
    with pytest.raises(NotImplementedError, match='ObjectRangeFilter'):
        TrainAugment.from_pipeline([dict(type='PointsRangeFilter', point_cloud_range=[-1, -1, -1, 1, 1, 1]),
                                    dict(type='ObjectRangeFilter', point_cloud_range=[-2, -2, -1, 2, 2, 1])])


def test_object_name_filter_is_host_side():
    from sst_amd.augment import TrainAugment
    aug = TrainAugment.from_pipeline(TRAIN[:6] + [dict(type='ObjectNameFilter', classes=['Car', 'Pedestrian'])] + TRAIN[6:])
    boxes = np.arange(21, dtype=F).reshape(3, 7)
    (b, l, pasted, rotate), = aug.assemble([boxes], [np.array([0, 2, 1])], None, 1)
    assert np.array_equal(b, boxes[[0, 2]]) and np.array_equal(l, [0, 1]) and pasted is None and rotate


def test_empty_box_tensor_is_not_rotated():
    """transforms_3d.py:609-614: points and boxes are rotated inside `if len(input_dict[key].tensor) != 0`, so a sample whose box
    tensor is empty after ObjectSample keeps its points unrotated; one pasted box is enough to rotate it"""
    from sst_amd.augment import TrainAugment
    aug = TrainAugment.from_pipeline(TRAIN)
    empty, one = np.zeros((0, 7), F), np.array([[1, 2, 0, 4, 2, 1.5, 0.3]], F)
    sampled = [None, dict(gt_bboxes_3d=one, gt_labels_3d=np.array([1]), points=np.zeros((3, 5), F))]
    asm = aug.assemble([empty, empty], [np.zeros(0, np.int64)] * 2, sampled, 2)
    assert [a[3] for a in asm] == [False, True]
    assert asm[1][0].shape == (1, 7) and np.array_equal(asm[1][1], [1]) and np.array_equal(asm[1][2], one)
    np.random.seed(3)
    p = aug.draw_params(2)
    rec = p.records(np.array([a[3] for a in asm]), aug.point_range, aug.shuffle)
    assert list(rec['rotate']) == [0, 1] and p.angle[0] != 0                 # the angle is drawn all the same (:600)
    pts = np.array([[3.0, 4.0, 0.5, 0.1, 0.2]], F)
    r0 = dict(flip_h=0, flip_v=0, rotate=0, shuffle=0, cos=rec['cos'][0], sin=rec['sin'][0], scale=F(1), trans=np.zeros(3, F),
              range=aug.point_range, seed=0, angle=rec['angle'][0])
    out, _ = R.augment_points(pts, 0, np.zeros((0, 6, 4), F), r0, 0)
    assert np.array_equal(out, pts)
    # test pipelines: no box field when GlobalRotScaleTrans runs -> rotated (:603-606)
    test = TrainAugment.from_pipeline([dict(type='MultiScaleFlipAug3D', flip=False, pts_scale_ratio=1, transforms=TRAIN[3:5])])
    assert test.assemble(None, None, None, 1)[0][3] is True


def test_nine_column_ground_truth_with_seven_column_pasted_boxes_is_refused():
    """transforms_3d.py:321-326 pads both to 10 columns; refused by name, with the reason"""
    from sst_amd.augment import TrainAugment
    aug = TrainAugment.from_pipeline(TRAIN)
    sampled = [dict(gt_bboxes_3d=np.zeros((2, 7), F), gt_labels_3d=np.zeros(2, np.int64), points=np.zeros((4, 5), F))]
    with pytest.raises(NotImplementedError, match='9-column ground truth and 7-column pasted boxes.*Waymo velocity'):
        aug.assemble([np.zeros((3, 9), F)], [np.zeros(3, np.int64)], sampled, 1)
    nine = [dict(gt_bboxes_3d=np.zeros((2, 9), F), gt_labels_3d=np.zeros(2, np.int64), points=np.zeros((4, 5), F))]
    (b, l, pasted, rotate), = aug.assemble([np.zeros((3, 9), F)], [np.zeros(3, np.int64)], nine, 1)
    assert b.shape == (5, 9) and pasted.shape == (2, 9) and rotate


def test_shuffle_key_restatement_is_splitmix64():
    """the hash against plain Python integers (arbitrary precision, reduced modulo 2^64)"""
    m = (1 << 64) - 1
    for seed, sample, n in ((0, 0, 5), (0xDEADBEEFCAFEF00D, 3, 70), (m, 2399, 4)):
        want = []
        for row in range(n):
            x = (seed + 0x9E3779B97F4A7C15 * (((sample << 32) | row) + 1)) & m
            x ^= x >> 30
            x = (x * 0xBF58476D1CE4E5B9) & m
            x ^= x >> 27
            x = (x * 0x94D049BB133111EB) & m
            x ^= x >> 31
            want.append(x >> 32)
        assert R.shuffle_keys(seed, sample, n).tolist() == want
