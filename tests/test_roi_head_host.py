"""The RoI head without a GPU: the restatement of tests/roi_head_ref.py against the reference's own methods
(tests/golden/roi_head_train.npz), the construction of GroupCorrectionHead / FullySparseBboxHead from every shipped config with a
``roi_head``, the refused keys, and the loud failures of the Python entry points on CPU tensors."""
import ast
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

import roi_head_ref as R

ROI_CONFIGS = sorted(os.path.relpath(p, os.path.join(GOLDEN, 'configs'))[:-len('.model.py')]
                     for d in ('fsd', 'fsdv2') for p in glob.glob(os.path.join(GOLDEN, 'configs', d, '*.model.py'))
                     if 'roi_head' in ast.literal_eval(open(p).read()))
CODE_WEIGHTS = [1.0, 1.0, 2.0, 0.5, 0.5, 0.25, 3.0]
# case -> (SmoothL1 beta, rcnn_code_weights, corner_loss_only_car); every case has its own nonempty mask in the golden
LOSS_CASES = {'main': (0.0, None, True), 'smooth': (1.0 / 9.0, CODE_WEIGHTS, False), 'nopos': (0.0, None, True),
              'nocar': (0.0, None, True)}
BATCH = 3


def loss_kwargs(case):
    beta, code_weight, only_car = LOSS_CASES[case]
    return dict(loss_weights=(1.0, 2.0, 1.0), beta=beta, code_weight=code_weight, with_corner=True, car_index=0 if only_car else -1)


@pytest.fixture(scope='module')
def gold():
    return load_golden('roi_head_train.npz')


def gold_scene(gold):
    """-> ((proposals, proposal labels, boxes, box labels) per sample, keys)"""
    return tuple([gold[f'{k}{s}'] for s in range(BATCH)] for k in ('props', 'plabels', 'gts', 'glabels')), gold['keys']


def gold_rows(gold):
    """the reference's sampled rows, concatenated over the samples"""
    return {k: gold['rows_' + k] for k in ('src', 'gt_index', 'labels', 'reg_mask', 'rois', 'iou_f32', 'iou_f64', 'soft_label_f32',
                                           'soft_label_f64', 'targets_f32', 'targets_f64')}


@pytest.fixture(scope='module')
def restated(gold):
    scene, keys = gold_scene(gold)
    return {dt: R.assign_sample(*scene, R.WAYMO_CFG, keys, dt) for dt in (np.float32, np.float64)}


def test_restated_assignment_and_sampling_equal_the_reference(gold, restated):
    ref = gold_rows(gold)
    for dt, tag in ((np.float32, 'f32'), (np.float64, 'f64')):
        res = restated[dt]
        rows = R.compact(res)
        assert np.array_equal(res['counts'], gold['counts'])
        assert np.array_equal(res['assigned'], gold['assigned'])
        for k in ('src', 'gt_index', 'labels', 'reg_mask', 'rois'):
            assert np.array_equal(rows[k], ref[k]), (tag, k)
        assert np.array_equal(res['pool_sizes'][0], gold['pool_sizes0'])
        for k in ('iou', 'soft_label', 'targets'):
            err = np.abs(rows[k] - ref[f'{k}_{tag}']).max()
            # float32: the restated IoU carries the library's cap (an overlap cannot exceed either box), the reference's does
            # not; the cap moves a value towards the exact one, by no more than the float32 IoU is off: noise_iou.  The soft
            # label divides that by cls_pos_thr - cls_neg_thr >= 0.5
            f32_bound = {'iou': 2 * float(gold['noise_iou']), 'soft_label': 4 * float(gold['noise_iou']) + 2e-6, 'targets': 2e-6}[k]
            assert err <= (1e-12 if dt == np.float64 else f32_bound), (tag, k, err)
        # padding rows: zeros and -1
        num = R.WAYMO_CFG['num']
        for s in range(BATCH):
            pad = slice(s * num + int(res['counts'][s].sum()), (s + 1) * num)
            assert (res['src'][pad] == -1).all() and (res['gt_index'][pad] == -1).all() and (res['labels'][pad] == -1).all()
            assert not res['rois'][pad].any() and not res['targets'][pad].any() and not res['reg_mask'][pad].any()


def test_the_scene_holds_the_cases_the_head_must_get_right(gold, restated):
    scene, keys = gold_scene(gold)
    props, plabels, gts, glabels = scene
    num = R.WAYMO_CFG['num']
    assert len(props[0]) > num and 0 < len(props[2]) < num and len(props[1]) == 0          # more than num, fewer, none (fake box)
    assert len(gts[2]) == 0 and len(gts[0]) > 0 and len(gts[1]) > 0                         # a sample without ground truth
    assert (glabels[0] == -1).sum() == 1 and set(glabels[0]) >= {0, 1, 2}
    assert gold['counts'].tolist()[1] == [0, 1] and gold['counts'][2, 0] == 0 and gold['counts'][0].sum() == num
    sizes = gold['pool_sizes0']         # positives, negatives of piece 0, of piece 1
    expected = num - gold['counts'][0, 0]
    assert sizes[1] < int(expected * 0.8) and sizes[2] > expected - sizes[1]                # the carry, and a real choice in piece 1
    res = restated[np.float64]
    n0 = len(props[0])
    dup = gold['duplicate_pair']
    assert np.array_equal(props[0][dup[0]], props[0][dup[1]]) and res['assigned'][dup[0]] == res['assigned'][dup[1]] >= 0
    assert res['overlaps'][dup[0]].tobytes() == res['overlaps'][dup[1]].tobytes()
    col = res['overlaps'][:n0, res['assigned'][dup[0]]]
    assert col[dup[0]] == col.max()                                                         # a bit-equal tie at the column maximum
    rerouted = (res['assigned'][:n0] >= 0) & (res['assigned'][:n0] != res['argmax'][:n0])
    assert rerouted.any()                                                                   # best box A, sent to box B
    # no decision sits on a rounding error
    noise = float(gold['noise_iou'])
    margin = max(1e-4, 10 * noise)
    used = res['overlaps'][res['overlaps'] > 0]
    for thr in (0.45, 0.35, 0.55, 0.1, 0.8, 0.65, 0.2, 0.15):
        assert np.abs(used - thr).min() > margin, thr
    rows = R.compact(res)
    pos = rows['reg_mask'] == 1
    all_gts = np.concatenate(gts)
    yaw = R.canonical_yaw(rows['rois'][pos, 1:8], all_gts[rows['gt_index'][pos]])
    for edge in (np.pi / 2, np.pi, 3 * np.pi / 2):
        assert np.abs(yaw - edge).min() > 0.05
    assert 0 <= noise < 1e-5 and 0 <= float(gold['noise_targets']) < 1e-5 and 0 <= float(gold['noise_soft_label']) < 1e-4
    # the loss cases
    main, nopos, nocar = (gold[f'{c}_nonempty'] for c in ('main', 'nopos', 'nocar'))
    assert (pos & ~main).any() and (pos & main).any()                                       # a positive RoI left empty
    assert not (pos & nopos).any() and float(gold['nopos_f64_loss_bbox']) == 0 and float(gold['nopos_f64_loss_corner']) == 0
    assert (pos & nocar).any() and not (pos & nocar & (rows['labels'] == 0)).any()
    assert float(gold['nocar_f64_loss_corner']) == 0 and float(gold['nocar_f64_loss_bbox']) > 0
    for case in LOSS_CASES:
        kw = loss_kwargs(case)
        keep = pos & gold[f'{case}_nonempty'] & ((rows['labels'] == 0) | (kw['car_index'] < 0))
        if keep.any():
            bp = torch.as_tensor(gold['bbox_pred'].astype(np.float64))[torch.as_tensor(keep)]
            roi = torch.as_tensor(rows['rois'][keep, 1:8].astype(np.float64))
            d0, d1 = R.corner_distances(R.decode_rows(roi, bp), torch.as_tensor(all_gts[rows['gt_index'][keep], :7].astype(np.float64)))
            assert (torch.min(d0, d1) - 1).abs().min() > 1e-3 and (d0 - d1).abs().min() > 1e-3


@pytest.mark.parametrize('case', list(LOSS_CASES))
def test_restated_losses_and_gradients_equal_the_reference(gold, restated, case):
    rows = R.compact(restated[np.float64])
    got = R.losses(gold['cls_score'].astype(np.float32), gold['bbox_pred'].astype(np.float32), gold[f'{case}_nonempty'], rows,
                   gold['gts'], dtype=torch.float64, **loss_kwargs(case))
    for k in ('num_pos', 'num_neg', 'corner_rows'):
        assert got[k] == int(gold[f'{case}_{k}']), k
    for k in ('loss_cls', 'loss_bbox', 'loss_corner'):
        ref = float(gold[f'{case}_f64_{k}'])
        assert abs(got[k] - ref) <= 1e-12 * max(abs(ref), 1e-30), (k, got[k], ref)
        assert 0 <= float(gold[f'noise_{case}_{k}']) < 1e-5
    for k in ('d_cls', 'd_bbox'):
        ref = gold[f'{case}_f64_{k}']
        assert np.array_equal(got[k] != 0, ref != 0), k
        assert np.abs(got[k] - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-30), k
        assert 0 <= float(gold[f'noise_{case}_{k}']) < 1e-5


def test_restated_decode_and_keep_list_equal_the_reference(gold):
    import box_ops_ref as B
    boxes, scores, bev = R.decode(gold['test_rois'], gold['test_bbox_pred'].astype(np.float32), gold['test_cls_score'].astype(np.float32))
    assert np.abs(boxes - gold['test_boxes_f64']).max() <= 1e-12 * np.abs(gold['test_boxes_f64']).max()
    assert 0 <= float(gold['noise_test_boxes']) < 1e-5
    valid = np.nonzero(gold['test_valid'])[0]
    labels, prob = gold['test_labels'][valid], gold['test_scores'][valid]
    selected = []
    for k in range(3):      # multi_class_nms: score_thr 0.1, nms_thr 0.25, rotated
        idx = np.nonzero((prob >= np.float32(0.1)) & (labels == k))[0]
        if len(idx):
            order = np.argsort(-prob[idx], kind='stable')
            keep = B.nms_host(bev[valid][idx][order].astype(np.float32), 0.25)
            selected.append(idx[order][keep])
    assert np.array_equal(np.concatenate(selected), gold['test_selected']) and 5 < len(gold['test_selected']) < len(valid)
    assert not gold['test_valid'].all()


def _model_cfg(name):
    return ast.literal_eval(open(os.path.join(GOLDEN, 'configs', name + '.model.py')).read())


def _build(name):
    import sst_amd
    det = sst_amd.build_detector(_model_cfg(name))
    return det, sst_amd.build_head(dict(det.unbuilt['roi_head'], train_cfg=det.train_cfg['rcnn'], test_cfg=det.test_cfg['rcnn']))


@pytest.mark.parametrize('name', ROI_CONFIGS)
def test_both_heads_build_from_every_config_with_a_roi_head(name):
    import sst_amd
    assert len(ROI_CONFIGS) == 7
    det, head = _build(name)
    cfg = det.unbuilt['roi_head']
    assert isinstance(head, sst_amd.GroupCorrectionHead) and isinstance(head.bbox_head, sst_amd.FullySparseBboxHead)
    assert isinstance(head.roi_extractor, sst_amd.DynamicPointROIExtractor)
    assert isinstance(head.bbox_head.bbox_coder, sst_amd.DeltaXYZWLHRBBoxCoder) and head.bbox_head.box_code_size == 7
    bh = cfg['bbox_head']
    assert len(head.bbox_head.block_list) == bh['num_blocks'] and head.bbox_head.with_corner_loss == bh['with_corner_loss']
    assert head.assign_cfg['class_mask'] and len(head.assign_cfg['pos_iou_thr']) == cfg['num_classes']
    assert head.sample_cfg['num'] == det.train_cfg['rcnn']['sampler']['num']
    assert head.bbox_head.train_cfg is det.train_cfg['rcnn'] and head.bbox_head.test_cfg is det.test_cfg['rcnn']
    assert sorted(head.state_dict()) == sorted(open(os.path.join(GOLDEN, 'roi_head_state_dict_keys.txt')).read().split())
    sd = head.state_dict()
    end = sum(sum(c) for c in bh['feat_channels'])
    assert tuple(sd['bbox_head.conv_cls.0.0.weight'].shape) == (bh['cls_mlp'][0], end)
    assert tuple(sd[f'bbox_head.conv_reg.{len(bh["reg_mlp"])}.weight'].shape) == (7, bh['reg_mlp'][-1])
    assert tuple(sd[f'bbox_head.conv_cls.{len(bh["cls_mlp"])}.weight'].shape) == (1, bh['cls_mlp'][-1])
    # the detector keeps parking the head's config, exactly as before
    assert det.unbuilt['roi_head'] == _model_cfg(name)['roi_head']
    assert not any(k.startswith('roi_head.') for k in det.state_dict())


def _rcnn(**over):
    cfg = ast.literal_eval(repr(_model_cfg('fsd/fsd_waymoD1_1x')['train_cfg']['rcnn']))
    cfg.update(over)
    return cfg


def _roi_head_cfg(train_cfg=None, bbox_head=None, **over):
    cfg = dict(_model_cfg('fsd/fsd_waymoD1_1x')['roi_head'], train_cfg=_rcnn() if train_cfg is None else train_cfg, test_cfg=dict())
    cfg['bbox_head'] = dict(cfg['bbox_head'], num_blocks=1, in_channels=[24], feat_channels=[[8, 8]], rel_mlp_hidden_dims=[[8]],
                            rel_mlp_in_channels=[13], reg_mlp=[8], cls_mlp=[8], **(bbox_head or {}))
    cfg.update(over)
    return cfg


def _assigner(i, **over):
    cfg = _rcnn()
    cfg['assigner'][i].update(over)
    return cfg


def _sampler(**over):
    cfg = _rcnn()
    cfg['sampler'].update(over)
    return cfg


@pytest.mark.parametrize('match, cfg', [
    ('add_gt_as_proposals', lambda: _roi_head_cfg(_sampler(add_gt_as_proposals=True))),
    ('neg_pos_ub', lambda: _roi_head_cfg(_sampler(neg_pos_ub=3))),
    ('ignore_iof_thr', lambda: _roi_head_cfg(_assigner(1, ignore_iof_thr=0.5))),
    ('assigner type', lambda: _roi_head_cfg(_assigner(0, type='ATSSAssigner'))),
    ('sampler type', lambda: _roi_head_cfg(_sampler(type='RandomSampler'))),
    ('iou_calculator', lambda: _roi_head_cfg(_assigner(2, iou_calculator=dict(type='BboxOverlaps3D', coordinate='camera')))),
    ('iou_calculator', lambda: _roi_head_cfg(_assigner(2, iou_calculator=dict(type='BboxOverlapsNearest3D', coordinate='lidar')))),
    ('gt_max_assign_all', lambda: _roi_head_cfg(_assigner(0, gt_max_assign_all=False))),
    ('class_wise_box_weights', lambda: _roi_head_cfg(_rcnn(class_wise_box_weights=[1, 2, 2]))),
    ('loss_cls', lambda: _roi_head_cfg(bbox_head=dict(loss_cls=dict(type='FocalLoss', use_sigmoid=True)))),
    ('loss_cls', lambda: _roi_head_cfg(bbox_head=dict(loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False)))),
    ('loss_cls', lambda: _roi_head_cfg(bbox_head=dict(loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, reduction='none')))),
    ('loss_bbox', lambda: _roi_head_cfg(bbox_head=dict(loss_bbox=dict(type='MSELoss')))),
    ('loss_bbox', lambda: _roi_head_cfg(bbox_head=dict(loss_bbox=dict(type='SmoothL1Loss', beta=0.0)))),
    ('bbox_coder', lambda: _roi_head_cfg(bbox_head=dict(bbox_coder=dict(type='DeltaXYZWLHRBBoxCoder', code_size=9)))),
])
def test_what_is_not_built_is_refused_by_name(match, cfg):
    import sst_amd
    with pytest.raises(NotImplementedError, match=match):
        sst_amd.build_head(cfg())


def test_the_refusals_leave_the_shipped_forms_alone():
    import sst_amd
    head = sst_amd.build_head(_roi_head_cfg())
    assert head.bbox_head.smooth_l1_beta == 0.0 and head.bbox_head.loss_weights == [1.0, 2.0, 1.0]
    smooth = sst_amd.build_head(_roi_head_cfg(bbox_head=dict(loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=2.0))))
    assert abs(smooth.bbox_head.smooth_l1_beta - 1.0 / 9.0) < 1e-12
    single = sst_amd.build_head(_roi_head_cfg(_rcnn(assigner=_rcnn()['assigner'][0])))       # the single-dict assigner
    assert not single.assign_cfg['class_mask'] and single.assign_cfg['pos_iou_thr'] == [0.45]
    with pytest.raises(NotImplementedError, match='get_bboxes_from_tracklet'):
        head.bbox_head.get_bboxes_from_tracklet()
    assert head.bbox_head._car_index() == 0
    coder = sst_amd.BBOX_CODERS.build(dict(type='DeltaXYZWLHRBBoxCoder'))
    a, b = torch.rand(6, 7) + 0.5, torch.rand(6, 7) + 0.5
    assert coder.code_size == 7 and torch.allclose(coder.decode(a, coder.encode(a, b)), b, atol=1e-5)


def test_ops_raise_on_cpu_tensors():
    import sst_amd
    scene = R.make_scene(0, [6, 3], [2, 1])
    t = [[torch.as_tensor(x) for x in part] for part in scene]
    with pytest.raises(RuntimeError):
        sst_amd.roi_assign_sample(*t, **R.WAYMO_CFG)
    n = 4
    with pytest.raises(RuntimeError):
        sst_amd.roi_loss(torch.zeros(n, 1), torch.zeros(n, 7), torch.ones(n, dtype=torch.bool), torch.zeros(n, 8), torch.zeros(n),
                         torch.zeros(n, dtype=torch.uint8), torch.zeros(n, 7))
    with pytest.raises(RuntimeError):
        sst_amd.roi_decode(torch.zeros(n, 8), torch.zeros(n, 7), torch.zeros(n, 1))
    head = sst_amd.build_head(_roi_head_cfg())
    with pytest.raises(RuntimeError):
        head._assign_and_sample([(t[0][s], torch.zeros(len(t[0][s])), t[1][s]) for s in range(2)], t[2], t[3])
