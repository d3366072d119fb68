"""The CTRL tracklet pipeline without a GPU: tests/tracklet_augment_ref.py, the float32 restatement the kernels are pinned to
(tests/test_gpu_tracklet_augment.py), against tests/golden/tracklet_pipeline.npz - the arrays the REFERENCE's own classes produced
stage by stage (tests/golden/make_tracklet_pipeline.py; the generator takes out every input whose reference output lies within
1e-3 m of a range bound and asserts that none is left) - and the host side of sst_amd.tracklet_augment: the draws, the frame
matrices, the pipeline fixtures, the refusals and LiDARTracklet.remove.

Rule: every stage is fed the reference's own previous-stage output and is EQUAL bit for bit, except
  * the rotation: the bar tests/test_augment_host.py asserts for the same restated function (ROT_BAR_ULP);
  * the pose step: POSE_BAR_ULP below;
  * the library's frame matrices: max(4 x the reference's float32-vs-float64 gap, 1e-6) relative to the largest element."""
import ast
import os

import numpy as np
import pytest
import torch

import tracklet_augment_ref as R
from conftest import ROOT
from test_augment_host import ROT_BAR_ULP, _rot_err_ulp, _ulp
from test_configs_build import REF, load_config

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
FIXTURES = os.path.join(GOLDEN, 'configs', 'pipeline', 'ctrl')
NAMES = ('ctrl_veh_24e', 'ctrl_ped_24e', 'ctrl_cyc_12e')
F = np.float32
PROPS = ['yaw', 'size', 'score', 'length']
CASE_SEEDS = (11, 12, 13, 14)                     # CASES of the generator: np.random.seed before the chain of each case

# The pose step: x' = ((m0 x + m1 y) + m2 z) + m3 written out against torch's ``[x y z 1] @ mm.T``, a four-term float32 dot
# product whose summation order and use of fused multiply-add are the BLAS library's.  With u = 2^-24 and
# S = |m0 x| + |m1 y| + |m2 z| + |m3|, any order of the three additions, with or without fusing, leaves an error of at most
# gamma_4 S = 4u / (1 - 4u) S on either side (the classical bound for n = 4 terms; the term m3 * 1 is exact, which only helps).
# u S < ulp(S), so each side stays within 4 (1 + 5u) ulp(S) and the two sides within 8 ulp(S) of each other, up to a factor
# 1 + 3e-7: the derived ceiling is 8 ulp.  Measured on the golden (four train chains and four test chains, 57 to 1 168 points
# each, translations of the frame matrices up to about 100 m): 1.0 ulp.  Asserted: twice that, rounded up to a whole ulp.
POSE_MEASURED_ULP = 1.0
POSE_CEILING_ULP = 8.0
POSE_BAR_ULP = min(float(np.ceil(2 * POSE_MEASURED_ULP)), POSE_CEILING_ULP)
ROT_CEILING_ULP = 4.0                             # tests/test_augment_host.py: the derived ceiling of the restated rotation


@pytest.fixture(scope='module')
def golden():
    return R.load_golden(GOLDEN)


def cases(g):
    return [R.golden_case(g, k) for k in range(int(g['n_cases']))]


def record(r, rng6, shuffle=0, seed=0):
    """the kernels' record of a golden case, formed as sst_amd.augment.AugmentParams.records forms it"""
    angle = torch.tensor(np.float32(r['angle']))
    return dict(flip_h=int(r['flips'][0]), flip_v=int(r['flips'][1]), rotate=1, shuffle=shuffle, cos=torch.cos(angle).numpy(),
                sin=torch.sin(angle).numpy(), angle=angle.numpy(), scale=F(r['scale']), trans=r['trans'].astype(F),
                range=np.asarray(rng6, F), seed=seed)


def pose_unit(xyz, mats_per_point):
    m = np.abs(mats_per_point[:, :3, :].astype(np.float64))
    x = np.abs(xyz.astype(np.float64))
    s = m[:, :, 0] * x[:, None, 0] + m[:, :, 1] * x[:, None, 1] + m[:, :, 2] * x[:, None, 2] + m[:, :, 3]
    return _ulp(s.astype(F))


def pose_err_ulp(frames, mats, want):
    lens = np.array([len(f) for f in frames])
    of = np.repeat(np.arange(len(frames)), lens)
    rows = np.concatenate(frames)[:, :3]
    got = R.pose_points(rows, mats[of][:, :3, :])
    return float((np.abs(got.astype(np.float64) - want) / pose_unit(rows, mats[of])).max())


def kept_frames(r):
    head = int(np.nonzero(r['ts'] == r['cut_ts'][0])[0][0])
    return head, len(r['ts']) - head - len(r['cut_ts']), r['frames'][head:head + len(r['cut_ts'])]


# ------------------------------------------------------------------------------------------------ stage by stage
def test_stage_by_stage_against_the_reference_classes(golden):
    worst_rot = 0.0
    rng6 = golden['range']
    noise_max = golden['noise_max']
    for k, r in enumerate(cases(golden)):
        # the cut: the reference's draws under its seed, the kept frames and the values their frame indices keep
        np.random.seed(CASE_SEEDS[k])
        head, tail = R.cutting_draws(len(r['ts']), tuple(golden['cut_cfg']), np.random)
        values = R.cut_frames(len(r['ts']), head, tail)
        assert np.array_equal(r['ts'][values], r['cut_ts']) and (head + tail == 10) == (len(r['ts']) == 160)
        lens = r['frame_lens'][values]
        assert np.array_equal(lens, r['cut_lens'])
        assert np.array_equal(np.where(lens > 0, values, -1), r['cut_frame_values'])
        assert np.array_equal(np.repeat(values, lens), r['frame_inds'])                  # they start at `head`
        assert np.array_equal(r['boxes'][values], r['cut_boxes']) and np.array_equal(r['scores'][values], r['cut_scores'])
        # noise and decoration
        cons = bool(r['consistent'])
        assert r['u_center'].shape == ((3,) if cons else (len(values), 3)) and r['u_yaw'].shape == (len(values),)
        noised = R.noise_boxes(r['pose_boxes'], r['u_center'], noise_max[:3], r['u_size'], noise_max[3:6], r['u_yaw'], noise_max[6])
        assert np.array_equal(noised, r['noise_boxes'])
        deco = R.decoration(r['noise_boxes'], r['cut_scores'], PROPS, len(values))
        filled = lens > 0
        assert filled.sum() >= 1 and np.array_equal(deco[filled], r['deco'][filled])
        # points: flips, rotation, scale, translation, the range
        rec = record(r, rng6)
        fh, fv = rec['flip_h'], rec['flip_v']
        assert np.array_equal(R.flip_points(r['pose_points'], fh, fv), r['flip_points'])
        rot = R.rotate_points(r['flip_points'], rec['cos'], rec['sin'])
        assert np.array_equal(rot[:, 2], r['rot_points'][:, 2])
        worst_rot = max(worst_rot, _rot_err_ulp(rot, r['rot_points'], r['flip_points']))
        assert np.array_equal(R.scale_points(r['rot_points'], rec['scale']), r['scale_points'])
        assert np.array_equal(R.translate_points(r['scale_points'], rec['trans']), r['trans_points'])
        assert np.array_equal(R.in_range_3d(r['trans_points'], rec['range']), r['mask'])
        assert np.array_equal(R.in_range_3d(r['test_pose_points'], rec['range']), r['test_mask'])
        assert np.array_equal(r['frame_inds'][r['mask']], r['final_frame_inds'])
        # boxes of the tracklet and of its candidates (the candidates are neither cut nor noised)
        assert np.array_equal(R.flip_boxes(r['noise_boxes'], fh, fv), r['flip_boxes'])
        rot = R.rotate_boxes(r['flip_boxes'], rec['cos'], rec['sin'], rec['angle'])
        assert np.array_equal(rot[:, 2:], r['rot_boxes'][:, 2:])
        worst_rot = max(worst_rot, _rot_err_ulp(rot, r['rot_boxes'], r['flip_boxes']))
        assert np.array_equal(R.scale_boxes(r['rot_boxes'], rec['scale']), r['scale_boxes'])
        assert np.array_equal(R.translate_boxes(r['scale_boxes'], rec['trans']), r['trans_boxes'])
        assert len(r['cands']) == (0, 1, 2, 1)[k]
        for c in r['cands']:
            assert len(set(c['ts'].tolist()) - set(r['ts'].tolist())) > 0            # timestamps outside the tracklet
            assert np.array_equal(R.flip_boxes(c['pose_boxes'], fh, fv), c['flip_boxes'])
            rot = R.rotate_boxes(c['flip_boxes'], rec['cos'], rec['sin'], rec['angle'])
            assert np.array_equal(rot[:, 2:], c['rot_boxes'][:, 2:])
            worst_rot = max(worst_rot, _rot_err_ulp(rot, c['rot_boxes'], c['flip_boxes']))
            assert np.array_equal(R.translate_boxes(R.scale_boxes(c['rot_boxes'], rec['scale']), rec['trans']), c['trans_boxes'])
        assert float(r['rot_angle_attr']) == float(r['angle'])
    print(f'rotation: worst error {worst_rot} ulp of |x| + |y| (bar {ROT_BAR_ULP})')
    assert worst_rot <= ROT_BAR_ULP


def test_pose_step_within_the_derived_bar(golden):
    """the restatement with the golden's own matrices against the reference's points, train chains and test chains"""
    worst = 0.0
    for r in cases(golden):
        _, _, frames = kept_frames(r)
        worst = max(worst, pose_err_ulp(frames, r['mm'], r['pose_points']))
        worst = max(worst, pose_err_ulp(r['frames'], r['test_mm'], r['test_pose_points']))
    print(f'pose step: worst error {worst} ulp of |m0 x| + |m1 y| + |m2 z| + |m3| (measured {POSE_MEASURED_ULP}, bar {POSE_BAR_ULP}, '
          f'ceiling {POSE_CEILING_ULP})')
    assert worst <= POSE_BAR_ULP <= POSE_CEILING_ULP


def test_frame_matrices_within_the_reference_gap(golden):
    """sst_amd's one batched product per sample against the reference's frame-by-frame products"""
    from sst_amd.tracklet_augment import frame_matrices
    for r in cases(golden):
        head, tail, _ = kept_frames(r)
        poses = r['poses'][head:len(r['ts']) - tail]
        for want, got, gap in ((r['mm'], frame_matrices(poses[len(poses) // 2], list(poses)), r['gap_mm']),
                               (r['test_mm'], frame_matrices(r['poses'][len(r['poses']) // 2], list(r['poses'])), r['gap_test_mm'])):
            got = got.numpy()
            assert got.dtype == np.float32 and got.shape == want.shape
            err = np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()
            assert err <= max(4 * float(gap), 1e-6), (err, float(gap))
        for c in r['cands']:
            got = frame_matrices(poses[len(poses) // 2], list(c['poses'])).numpy()
            assert np.abs(got.astype(np.float64) - c['mm']).max() / np.abs(c['mm']).max() <= max(4 * float(r['gap_mm']), 1e-6)


# ------------------------------------------------------------------------------------------------ the host side of the library
def train_pipeline(cut=None, cons=False, props=PROPS, rng6=None, yaw_cons=False, size=True):
    cut = dict(ratio=0.0, max_length=150) if cut is None else cut
    return [dict(type='LoadTrackletPoints', load_dim=6, use_dim=5, max_points=1024, debug=False), dict(type='LoadTrackletAnnotations'),
            dict(type='TrackletCutting', **cut), dict(type='TrackletPoseTransform', concat=False),
            dict(type='TrackletNoise', center_noise_cfg=dict(max_noise=[0.2, 0.2, 0.1], consistent=cons),
                 size_noise_cfg=dict(max_noise=[0.2, 0.2, 0.1], consistent=cons) if size else None,
                 yaw_noise_cfg=dict(max_noise=0.2, consistent=yaw_cons)),
            dict(type='PointDecoration', properties=list(props), concat=True),
            dict(type='TrackletRandomFlip', flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
            dict(type='TrackletGlobalRotScaleTrans', rot_range=[-0.78539816, 0.78539816], scale_ratio_range=[0.95, 1.05],
                 translation_std=[0, 0, 0.2]),
            dict(type='PointsRangeFilter', point_cloud_range=[-24.0, -24.0, -2.5, 24.0, 24.0, 3.0] if rng6 is None else list(rng6)),
            dict(type='PointShuffle'), dict(type='TrackletFormatBundle', class_names=['Car']),
            dict(type='Collect3D', keys=['points', 'pts_frame_inds', 'tracklet', 'gt_tracklet_candidates'])]


def library_tracklet(boxes, ts, scores, poses, name='t'):
    import sst_amd
    t = sst_amd.LiDARTracklet('seg', name, 1, True, torch.as_tensor(np.asarray(boxes, F)), [int(x) for x in ts], [float(s) for s in scores])
    t.freeze()
    t.pose_list = [torch.as_tensor(np.asarray(p, F)) for p in poses]
    return t


def golden_batch(r):
    """(tracklet, candidates, params) of a golden case for sst_amd.tracklet_augment"""
    from sst_amd.tracklet_augment import TrackletParams
    trk = library_tracklet(r['boxes'], r['ts'], r['scores'], r['poses'])
    cands = [library_tracklet(c['boxes'], c['ts'], [1.0] * len(c['ts']), c['poses'], f'c{j}') for j, c in enumerate(r['cands'])]
    p = TrackletParams(1)
    head, tail, _ = kept_frames(r)
    p.cut[0], p.center_noise[0], p.size_noise[0], p.yaw_noise[0] = (head, tail), r['u_center'], r['u_size'], r['u_yaw']
    p.flip_h[0], p.flip_v[0], p.angle[0], p.scale[0], p.trans[0] = r['flips'][0], r['flips'][1], r['angle'], r['scale'], r['trans']
    return trk, cands, p


def test_host_side_of_the_library_against_the_reference(golden):
    """prepare_boxes (the cut, ONE batched pose product, the noise, the decoration values): what does not depend on the frame
    matrices is equal, what does stays within max(4 x the reference's own gap, 1e-6); the records are the restatement's"""
    from sst_amd.tracklet_augment import TrackletAugment
    for k, r in enumerate(cases(golden)):
        aug = TrackletAugment.from_pipeline(train_pipeline(cons=bool(r['consistent'])))
        trk, cands, p = golden_batch(r)
        per_sample, boxes, ranges = aug.prepare_boxes([trk], [cands], p)
        mm, deco, values, (head, n), center = per_sample[0]
        assert np.array_equal(trk.ts_list, r['cut_ts']) and n == len(r['cut_ts']) and np.array_equal(values, np.arange(head, head + n))
        assert np.array_equal(center.numpy(), r['shared_pose'])
        own = boxes[ranges[0][0][0]:ranges[0][0][1]].numpy()
        rel = lambda a, b: np.abs(a.astype(np.float64) - b).max() / np.abs(b).max()          # noqa: E731
        assert rel(own, r['noise_boxes']) <= max(4 * float(r['gap_noise_boxes']), 1e-6)
        assert np.array_equal(own[:, 3:6], r['noise_boxes'][:, 3:6])                          # the sizes never see a matrix
        assert np.array_equal(deco.numpy()[:, 1:], R.decoration(r['noise_boxes'], r['cut_scores'], PROPS, n)[:, 1:])
        assert np.array_equal(deco.numpy(), R.decoration(own, r['cut_scores'], PROPS, n))
        for c, (r0, r1) in zip(r['cands'], ranges[0][1:]):
            assert rel(boxes[r0:r1].numpy(), c['pose_boxes']) <= max(4 * float(r['gap_pose_boxes']), 1e-6)
        rec = aug.records(p)[0]
        want = record(r, golden['range'], shuffle=1)
        for key in ('flip_h', 'flip_v', 'rotate', 'shuffle', 'cos', 'sin', 'angle', 'scale', 'trans', 'range'):
            assert np.array_equal(rec[key], want[key]), key


def test_end_to_end_restatement_against_the_reference_chain(golden):
    """the restated chain with the golden's matrices: the surviving rows are the reference's, in its order, their frame indices
    too.  The two sides rotate DIFFERENT inputs here (they differ by the pose step's error), so the rotation contributes its
    derived ceiling (4 ulp of |x| + |y|: 1.5 per side for two products and a sum, tests/test_augment_host.py) and the pose error
    of x and of y, each weighted by a cosine or sine of at most 1; the scale (<= 1.05) and the translation add one rounding on
    each side.  z goes through the scale and the translation only.  Every other column is bit-equal"""
    for k, r in enumerate(cases(golden)):
        head, tail, frames = kept_frames(r)
        rec = record(r, golden['range'])
        values = R.cut_frames(len(r['ts']), head, tail)
        deco = np.nan_to_num(r['deco'])
        out, fi, idx = R.augment_sample(frames, r['mm'], deco, values, rec, 0)
        assert np.array_equal(idx, np.nonzero(r['mask'])[0]) and np.array_equal(fi, r['final_frame_inds'])
        rows = np.concatenate(frames)
        of = np.repeat(np.arange(len(frames)), [len(f) for f in frames])
        pose_tol = POSE_BAR_ULP * pose_unit(rows[:, :3], r['mm'][of])
        rot_tol = ROT_CEILING_ULP * _ulp(np.abs(r['flip_points'][:, 0]) + np.abs(r['flip_points'][:, 1]))
        tol_xy = 1.05 * (pose_tol[:, :2].sum(1) + rot_tol) + _ulp(r['scale_points'][:, :2]).max(1) + _ulp(r['trans_points'][:, :2]).max(1)
        tol_z = 1.05 * pose_tol[:, 2] + _ulp(r['scale_points'][:, 2]) + _ulp(r['trans_points'][:, 2])
        m = r['mask']
        assert (np.abs(out[:, :2].astype(np.float64) - r['trans_points'][m][:, :2]) <= tol_xy[m][:, None]).all()
        assert (np.abs(out[:, 2].astype(np.float64) - r['trans_points'][m][:, 2]) <= tol_z[m]).all()
        assert np.array_equal(out[:, 3:5], rows[m][:, 3:5]) and np.array_equal(out[:, 5:], deco[of][m])


# ------------------------------------------------------------------------------------------------ the draws
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_draw_params_follows_the_reference_draws(golden, seed):
    """np.random.seed(k) and torch.manual_seed(k), five tracklets of 3 (below min_length: the first draw is short-circuited),
    37, 160, 150 and 8 frames: the cut, the torch.rand draws and their shapes, the flips, the angle, the scale and the
    translation equal what the reference's transforms, run from source sample after sample, drew"""
    from sst_amd.tracklet_augment import TrackletAugment
    min_length, ratio, max_cut_ratio, max_length, cons = golden[f'draw{seed}_cfg']
    cut = dict(min_length=int(min_length), ratio=float(ratio), max_cut_ratio=float(max_cut_ratio), max_length=int(max_length))
    aug = TrackletAugment.from_pipeline(train_pipeline(cut=cut, cons=bool(cons), size=False))
    lens = golden['draw_lens'].tolist()
    np.random.seed(seed)
    torch.manual_seed(seed)
    p = aug.draw_params(lens)
    want = golden[f'draw{seed}']
    assert np.array_equal(np.asarray(p.cut, np.float64), want[:, :2])
    assert np.array_equal(p.flip_h.astype(np.float64), want[:, 2]) and np.array_equal(p.flip_v.astype(np.float64), want[:, 3])
    assert np.array_equal(p.angle, want[:, 4]) and np.array_equal(p.scale, want[:, 5]) and np.array_equal(p.trans, want[:, 6:9])
    for i, n in enumerate(lens):
        kept = n - sum(p.cut[i])
        uc, uy = golden[f'draw{seed}_s{i}_u_center'], golden[f'draw{seed}_s{i}_u_yaw']
        assert p.center_noise[i].shape == uc.shape == ((3,) if cons else (kept, 3)) and np.array_equal(p.center_noise[i], uc)
        assert p.size_noise[i] is None and p.yaw_noise[i].shape == uy.shape == (kept,) and np.array_equal(p.yaw_noise[i], uy)
    assert want[0, 9] == 5 and want[1, 9] >= 6                      # np.random calls of the reference: none by the cut of the short tracklet
    assert len(set(int(s) for s in p.seed)) == len(lens)
    rs = np.random.RandomState(seed)                                 # a RandomState and a generator draw the same
    q = aug.draw_params(lens, rs, torch.Generator().manual_seed(seed))
    assert np.array_equal(q.angle, p.angle) and np.array_equal(q.seed, p.seed) and q.cut == p.cut
    assert all(np.array_equal(a, b) for a, b in zip(q.center_noise, p.center_noise))


def test_consistent_yaw_draws_one_number():
    from sst_amd.tracklet_augment import TrackletAugment
    aug = TrackletAugment.from_pipeline(train_pipeline(cons=True, yaw_cons=True))
    p = aug.draw_params([9], np.random.RandomState(0), torch.Generator().manual_seed(0))
    assert p.center_noise[0].shape == (3,) and p.size_noise[0].shape == (3,) and p.yaw_noise[0].shape == (1,)
    test = TrackletAugment.from_pipeline([s for s in train_pipeline() if s['type'] in (
        'LoadTrackletPoints', 'TrackletPoseTransform', 'PointDecoration', 'PointsRangeFilter', 'PointShuffle')])
    state = np.random.RandomState(3).get_state()
    rs = np.random.RandomState(3)
    q = test.draw_params([9, 200], rs)                               # a test pipeline draws the seeds only
    assert q.cut == [(0, 0)] * 2 and q.yaw_noise == [None] * 2 and not q.flip_h.any() and not q.angle.any() and (q.scale == 1).all()
    rs2 = np.random.RandomState(3)
    rs2.set_state(state)
    assert int(q.seed[0]) == (int(rs2.randint(0, 2 ** 32)) << 32) | int(rs2.randint(0, 2 ** 32))


# ------------------------------------------------------------------------------------------------ fixtures and refusals
def fixture(name):
    return ast.literal_eval(open(os.path.join(FIXTURES, name + '.pipeline.py')).read())


@pytest.mark.parametrize('name', NAMES)
def test_fixture_equals_the_config_text(name):
    path = os.path.join(REF, 'configs', 'ctrl', name + '.py')
    if not os.path.exists(path):
        pytest.skip('the reference tree is not on this machine')
    cfg = load_config(path)
    assert {k: cfg[k] for k in ('train_pipeline', 'test_pipeline')} == fixture(name)


@pytest.mark.parametrize('name', NAMES)
def test_every_shipped_pipeline_builds(name):
    from sst_amd.tracklet_augment import TrackletAugment
    cfg = fixture(name)
    train = TrackletAugment.from_pipeline(cfg['train_pipeline'])
    assert train.use_dim == 5 and train.pose and train.properties == ('yaw', 'size', 'score') and train.deco == 5
    assert train.flip == (0.5, 0.5) and train.rst == ([-0.78539816, 0.78539816], [0.95, 1.05], [0, 0, 0.2]) and train.shuffle
    if name == 'ctrl_ped_24e':                                       # the pedestrian config has no TrackletNoise
        assert train.noise is None
    else:
        assert train.noise[2] == (0.2, False) and train.noise[1] == ([0.2, 0.2, 0.1], False)
        assert train.noise[0] == ([0.2, 0.2, 0.1] if name == 'ctrl_veh_24e' else [0.4, 0.4, 0.2], False)
    assert (train.cutting == (5, 0.0, 0.5, 150)) == (name == 'ctrl_veh_24e') and (train.cutting is None) == (name != 'ctrl_veh_24e')
    assert np.array_equal(train.point_range, np.array([-204.7, -204.7, -3.99, 204.7, 204.7, 7.99], F))
    test = TrackletAugment.from_pipeline(cfg['test_pipeline'])
    assert test.cutting is None and test.noise is None and test.flip is None and test.rst is None and test.shuffle and test.deco == 5
    assert np.array_equal(test.point_range, train.point_range)
    rec = test.records(test.draw_params([4, 2], np.random.RandomState(0)))
    assert not rec['rotate'].any() and (rec['scale'] == 1).all() and np.signbit(rec['trans']).all() and not rec['trans'].any()


def _with(step, at='TrackletNoise', replace=False):
    steps = train_pipeline()
    i = [s['type'] for s in steps].index(at)
    return steps[:i] + [step] + steps[i + (1 if replace else 0):]


@pytest.mark.parametrize('steps,name', [
    (_with(dict(type='FrameDropout', drop_ratio=0.1)), 'FrameDropout'),
    (_with(dict(type='TrackletScaling')), 'TrackletScaling'),
    (_with(dict(type='MultiScaleFlipAug3D', transforms=[]), 'TrackletRandomFlip'), 'MultiScaleFlipAug3D'),
    (_with(dict(type='PointDecoration', properties=['yaw', 'center_offset']), 'PointDecoration', True), 'center_offset'),
    (_with(dict(type='TrackletPoseTransform', concat=False, centering=True), 'TrackletPoseTransform', True), 'centering=True'),
    (_with(dict(type='TrackletGlobalRotScaleTrans', shift_height=True), 'TrackletGlobalRotScaleTrans', True), 'shift_height=True'),
    (_with(dict(type='RandomFlip3D', sync_2d=False), 'TrackletRandomFlip', True), 'RandomFlip3D'),
    (_with(dict(type='ObjectSample', db_sampler=dict())), 'ObjectSample'),
    (_with(dict(type='PointDecoration', properties=['yaw', 'size', 'score', 'length', 'size', 'size']), 'PointDecoration', True),
     'SST_TRK_AUG_MAX_DECO'),
])
def test_refusals_name_the_transform(steps, name):
    from sst_amd.tracklet_augment import TrackletAugment
    with pytest.raises(NotImplementedError, match=name):
        TrackletAugment.from_pipeline(steps)


def test_steps_out_of_order_are_refused_by_name():
    from sst_amd.tracklet_augment import TrackletAugment
    steps = train_pipeline()
    names = [s['type'] for s in steps]
    for a, b in (('TrackletNoise', 'PointDecoration'), ('TrackletRandomFlip', 'TrackletGlobalRotScaleTrans'),
                 ('TrackletCutting', 'TrackletPoseTransform'), ('PointsRangeFilter', 'PointShuffle')):
        swapped = list(steps)
        i, j = names.index(a), names.index(b)
        swapped[i], swapped[j] = swapped[j], swapped[i]
        with pytest.raises(NotImplementedError, match=a):
            TrackletAugment.from_pipeline(swapped)
    with pytest.raises(NotImplementedError, match='TrackletPoseTransform'):
        TrackletAugment.from_pipeline([s for s in steps if s['type'] != 'TrackletPoseTransform'])
    # the detection module keeps refusing the tracklet steps, and the tracklet methods it refuses stay refused
    from sst_amd.augment import TrainAugment
    with pytest.raises(NotImplementedError, match='TrackletRandomFlip'):
        TrainAugment.from_pipeline([dict(type='TrackletRandomFlip')])


def test_no_cpu_path():
    from sst_amd.tracklet_augment import TrackletAugment
    if torch.cuda.is_available():
        pytest.skip('a GPU is present: tests/test_gpu_tracklet_augment.py runs the call')
    aug = TrackletAugment.from_pipeline(train_pipeline())
    t = library_tracklet(np.zeros((1, 7), F) + 1, [10 ** 15], [0.5], [np.eye(4)])
    with pytest.raises(RuntimeError, match='no CPU path'):
        aug([[np.zeros((3, 5), F)]], [t], [[]])


# ------------------------------------------------------------------------------------------------ LiDARTracklet.remove
@pytest.mark.parametrize('k', [0, 1, 2])
def test_remove_equals_the_reference(golden, k):
    import sst_amd
    r = R.golden_case(golden, k)
    t = library_tracklet(r['boxes'], r['ts'], r['scores'], r['poses'])
    keep_idx = t.remove(r['remove_ts'].tolist())
    assert 'remove' not in sst_amd.tracklet.REFUSED_METHODS
    assert keep_idx == r['remove_keep_idx'].tolist() and t.ts_list == r['remove_left_ts'].tolist() and len(t) == len(keep_idx)
    assert np.array_equal(t.boxes.numpy(), r['remove_boxes']) and np.array_equal(np.asarray(t.score_list), r['remove_scores'])
    assert np.array_equal(np.stack([p.numpy() for p in t.pose_list]), r['remove_poses'])
    assert [t.ts2index[ts] for ts in t.ts_list] == r['remove_index'].tolist() and t.ts_set == set(t.ts_list) and t.frozen
    assert len(t.box_list) == len(keep_idx) and t.remove(None) == list(range(len(keep_idx)))
