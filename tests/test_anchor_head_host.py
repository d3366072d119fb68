"""Anchor3DHead without a GPU: the restatement of tests/anchor_head_ref.py against the reference's golden
(tests/golden/anchor_head_train.npz), the anchor generators, the shipped configs, the refusals and the CPU-tensor errors."""
import ast
import copy
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

import anchor_head_ref as R

SHIPPED = sorted(glob.glob(os.path.join(GOLDEN, 'configs', 'sst', '*.model.py'))) + [
    os.path.join(GOLDEN, 'configs', 'sst_refactor', 'sst_waymoD5_1x_3class_8heads_v2.model.py')]


@pytest.fixture(scope='module')
def gold():
    return load_golden('anchor_head_train.npz')


def scene(gold, case):
    sel = [R.case_labels(case, gold[f'labels{s}']) for s in range(3)]
    return [gold[f'boxes{s}'][k] for s, (k, _) in enumerate(sel)], [l[k] for k, l in sel]


_RESTATED = {}


def restated(gold, case):
    """the restated targets of a golden case, computed once and left unchanged"""
    if case not in _RESTATED:
        cfg = R.CASES[case]
        grid = R.make_grid(cfg['anchor_generator'], R.H, R.W)
        boxes, labels = scene(gold, case)
        _RESTATED[case] = (grid,) + R.batch_targets(grid, boxes, labels, cfg)
    return _RESTATED[case]


@pytest.mark.parametrize('case', list(R.CASES))
def test_restated_targets_equal_the_reference(gold, case):
    grid, dense, per_sample, n_pos, n_neg = restated(gold, case)
    assert np.array_equal(np.stack([p[0].reshape(-1) for p in per_sample]), gold[f'tgt_{case}_assigned'])
    for k in ('labels', 'label_weights', 'bbox_weights', 'dir_targets', 'dir_weights'):
        assert dense[k].dtype == gold[f'tgt_{case}_{k}'].dtype and np.array_equal(dense[k], gold[f'tgt_{case}_{k}']), k
    assert (n_pos, n_neg) == (int(gold[f'tgt_{case}_num_total_pos']), int(gold[f'tgt_{case}_num_total_neg']))
    got = np.stack([p[1].reshape(-1) for p in per_sample])
    assert np.array_equal(got.view(np.int32), gold[f'tgt_{case}_max_iou'].view(np.int32)), 'per-anchor maximum IoU, bit for bit'
    want = gold[f'tgt_{case}_bbox_targets']
    plain = [0, 1, 2, 6]
    assert np.array_equal(dense['bbox_targets'][..., plain].view(np.int32), want[..., plain].view(np.int32))
    d = R.ulp_distance(dense['bbox_targets'][..., 3:6], want[..., 3:6]).max()
    print(f'{case}: log columns max ulp distance {d}')
    assert d <= 1                                      # torch.log on both sides; its vector and scalar paths may round apart
    assert (gold[f'tgt_{case}_assigned'][1] == -1).all(), 'the empty sample is all background'


def test_the_scene_holds_what_it_is_meant_to(gold):
    grid, dense, per_sample, _, _ = restated(gold, 'shipped')
    assigned, max_iou, gt_max = per_sample[0]
    assert (assigned == 0).sum() == 0 and gt_max[:, 0].max() == 0                      # the box outside the range
    assert np.float32(0.3) <= gt_max[1, 3] < np.float32(0.5) and (assigned == 3).sum() >= 1   # a low-quality match
    tie = (max_iou[:, :, 2, :] == gt_max[2, 4]) & (assigned[:, :, 2, :] == 4)
    assert tie.sum() == 2                                                              # two anchors at exactly equal IoU
    assert (assigned == -2).sum() > 0 and (gold['tgt_per_class_assigned'] != gold['tgt_shipped_assigned']).any()


@pytest.mark.parametrize('case', list(R.CASES))
def test_restated_losses_equal_the_reference(gold, case):
    cfg = R.CASES[case]
    grid, dense, _, n_pos, _ = restated(gold, case)
    tag = f'{grid.ns * grid.nr}x{cfg["num_classes"]}'
    maps = [gold[f'maps_{tag}_{k}'].astype(np.float32) for k in ('cls', 'box', 'dir')]
    boxes, labels = scene(gold, case)
    dense64 = R.batch_targets(grid, boxes, labels, cfg, np.float64)[0]
    r = R.loss_and_grads(*maps, dense64, n_pos, cfg)
    for k in ('loss_cls', 'loss_bbox', 'loss_dir'):
        want = float(gold[f'loss_{case}_f64_{k}'])
        print(case, k, r[k], want)
        assert abs(r[k] - want) <= 1e-12 * abs(want)
    want = gold[f'loss_{case}_f64_d_cls_8th']
    assert np.abs(r['d_cls'].reshape(-1)[::8] - want).max() <= 1e-12 * np.abs(want).max()
    for k in ('d_bbox', 'd_dir'):
        want = gold[f'loss_{case}_f64_{k}']
        assert np.abs(r[k] - want).max() <= 1e-12 * np.abs(want).max()
        assert np.array_equal(r[k] != 0, want != 0)


@pytest.mark.parametrize('case', ['shipped', 'smooth', 'ped_cyc'])
def test_restated_detections_equal_the_reference(gold, case):
    cfg = R.CASES[case]
    grid = R.make_grid(cfg['anchor_generator'], R.H, R.W)
    tag = f'{grid.ns * grid.nr}x{cfg["num_classes"]}'
    maps = [gold[f'maps_{tag}_{k}'].astype(np.float32) for k in ('cls', 'box', 'dir')]
    for s in range(3):
        boxes, scores, labels = R.get_bboxes_single(grid, maps[0][s], maps[1][s], maps[2][s], cfg)
        assert np.array_equal(labels, gold[f'det_{case}_s{s}_labels']) and np.array_equal(scores, gold[f'det_{case}_s{s}_scores'])
        assert R.ulp_distance(boxes, gold[f'det_{case}_s{s}_bboxes']).max() <= 1
    assert (grid.ns * grid.nr * R.H * R.W > cfg['test_cfg']['nms_pre']) == (case == 'smooth')


def test_generators_give_the_reference_anchors(gold):
    import sst_amd
    gen = sst_amd.build_anchor_generator(R.generator_cfg())
    assert gen.num_base_anchors == 6 and gen.num_levels == 1
    anchors = gen.grid_anchors([(R.H, R.W)], device='cpu')[0]
    assert tuple(anchors.shape) == (1, R.H, R.W, 3, 2, 7)
    assert np.array_equal(anchors[0].numpy().view(np.int32), gold['anchors'].view(np.int32))
    assert gen.grid((R.H, R.W), 'cpu') is gen.grid((R.H, R.W), 'cpu'), 'the tables are formed once per feature-map size'
    flat = sst_amd.build_anchor_generator(dict(R.generator_cfg(), reshape_out=True)).grid_anchors([(R.H, R.W)], device='cpu')[0]
    assert torch.equal(flat, anchors.reshape(-1, 7))
    # Anchor3DRangeGenerator: torch.linspace between the ends of the range, one range for all sizes
    plain = sst_amd.build_anchor_generator(dict(type='Anchor3DRangeGenerator', ranges=[[0, -39.68, -1.78, 69.12, 39.68, -1.78]],
                                                sizes=[[1.6, 3.9, 1.56], [0.6, 0.8, 1.73]], rotations=[0, 1.57],
                                                reshape_out=False, size_per_range=False))
    a = plain.grid_anchors([(5, 7)], device='cpu')[0]
    assert tuple(a.shape) == (1, 5, 7, 2, 2, 7) and plain.num_base_anchors == 4
    assert torch.equal(a[0, 2, :, 1, 0, 0], torch.linspace(0, 69.12, 7)) and torch.equal(a[0, :, 3, 0, 1, 1], torch.linspace(-39.68, 39.68, 5))
    assert torch.equal(a[0, 1, 1, :, 0, 3:6], torch.tensor([[1.6, 3.9, 1.56], [0.6, 0.8, 1.73]])) and float(a[0, 0, 0, 0, 1, 6]) == np.float32(1.57)
    with pytest.raises(NotImplementedError, match='custom_values'):
        sst_amd.build_anchor_generator(dict(R.generator_cfg(), custom_values=[0, 0]))


REF_HEAD_KEYS = ['conv_cls.bias', 'conv_cls.weight', 'conv_dir_cls.bias', 'conv_dir_cls.weight', 'conv_reg.bias', 'conv_reg.weight']
REF_NECK_KEYS = ['deblocks.0.0.weight', 'deblocks.0.1.bias', 'deblocks.0.1.num_batches_tracked', 'deblocks.0.1.running_mean',
                 'deblocks.0.1.running_var', 'deblocks.0.1.weight']


@pytest.mark.parametrize('path', SHIPPED, ids=[os.path.basename(p)[:-len('.model.py')] for p in SHIPPED])
def test_shipped_configs_build_neck_and_head(path):
    import sst_amd
    det = sst_amd.build_detector(ast.literal_eval(open(path).read()))
    before = copy.deepcopy(det.unbuilt)
    neck = sst_amd.build_neck(det.unbuilt['neck'])
    head = sst_amd.build_head(dict(det.unbuilt['bbox_head'], train_cfg=det.train_cfg, test_cfg=det.test_cfg))
    assert det.unbuilt == before and set(det.unbuilt) == {'neck', 'bbox_head'}
    assert sorted(head.state_dict()) == REF_HEAD_KEYS and sorted(neck.state_dict()) == REF_NECK_KEYS
    cfg = det.unbuilt['bbox_head']
    n_a = len(cfg['anchor_generator']['sizes']) * len(cfg['anchor_generator']['rotations'])
    assert head.num_anchors == n_a and head.conv_cls.out_channels == n_a * cfg['num_classes']
    assert head.conv_reg.out_channels == n_a * 7 and head.conv_dir_cls.out_channels == n_a * 2
    assert isinstance(neck.deblocks[0][0], torch.nn.ConvTranspose2d) and neck.deblocks[0][0].bias is None
    # the reference's initialisation: Normal(0, 0.01), conv_cls' bias from bias_prob 0.01
    assert abs(float(head.conv_cls.bias.detach()[0]) + np.log(99.0)) < 1e-6 and float(head.conv_reg.bias.detach().abs().max()) == 0
    assert 0.005 < float(head.conv_reg.weight.detach().std()) < 0.02
    out = neck([torch.randn(2, det.unbuilt['neck']['in_channels'][0], 6, 5)])
    assert len(out) == 1 and tuple(out[0].shape) == (2, sum(det.unbuilt['neck']['out_channels']), 6, 5)
    if det.test_cfg.get('wnms'):
        with pytest.raises(NotImplementedError, match='wnms'):
            head.get_bboxes([torch.zeros(1, 2, 4, 4)], [torch.zeros(1, 14, 4, 4)], [torch.zeros(1, 4, 4, 4)], [dict()])


def test_secondfpn_layers():
    import sst_amd
    neck = sst_amd.build_neck(dict(type='SECONDFPN', in_channels=[4, 6, 8], out_channels=[5, 5, 5], upsample_strides=[1, 2, 4],
                                   norm_cfg=dict(type='BN', eps=1e-3, momentum=0.01), use_conv_for_no_stride=True))
    assert isinstance(neck.deblocks[0][0], torch.nn.Conv2d) and isinstance(neck.deblocks[1][0], torch.nn.ConvTranspose2d)
    assert neck.deblocks[2][0].stride == (4, 4) and isinstance(neck.deblocks[0][2], torch.nn.ReLU)
    out = neck([torch.randn(1, 4, 8, 8), torch.randn(1, 6, 4, 4), torch.randn(1, 8, 2, 2)])
    assert tuple(out[0].shape) == (1, 15, 8, 8)


def _head_cfg(**kw):
    cfg = dict(R.CASES['shipped'], type='Anchor3DHead', in_channels=8, feat_channels=8)
    cfg.update(kw)
    return cfg


def _train(**kw):
    a = [dict(x, **kw) for x in R.ASSIGN_3]
    return dict(R.CASES['shipped']['train_cfg'], assigner=a)


@pytest.mark.parametrize('key, cfg', [
    ('assigner', _head_cfg(train_cfg=_train(type='ATSSAssigner'))),
    ('iou_calculator', _head_cfg(train_cfg=_train(iou_calculator=dict(type='BboxOverlaps3D', coordinate='lidar')))),
    ('iou_calculator', _head_cfg(train_cfg=_train(iou_calculator=dict(type='BboxOverlapsNearest3D', coordinate='camera')))),
    ('ignore_iof_thr', _head_cfg(train_cfg=_train(ignore_iof_thr=0.5))),
    ('min_pos_iou', _head_cfg(train_cfg=_train(min_pos_iou=0.0))),
    ('match_low_quality', _head_cfg(train_cfg=_train(match_low_quality=False))),
    ('gt_max_assign_all', _head_cfg(train_cfg=_train(gt_max_assign_all=False))),
    ('assigner_per_size', _head_cfg(assigner_per_size=True)),
    ('loss_cls', _head_cfg(loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0))),
    ('use_sigmoid', _head_cfg(loss_cls=dict(type='FocalLoss', use_sigmoid=False))),
    ('loss_bbox', _head_cfg(loss_bbox=dict(type='GIoULoss'))),
    ('loss_dir', _head_cfg(loss_dir=dict(type='CrossEntropyLoss', use_sigmoid=True))),
    ('scales', _head_cfg(anchor_generator=dict(R.generator_cfg(), scales=[1, 2]))),
    ('custom_values', _head_cfg(anchor_generator=dict(R.generator_cfg(), custom_values=[0, 0]))),
    ('code_size', _head_cfg(bbox_coder=dict(type='DeltaXYZWLHRBBoxCoder', code_size=9))),
])
def test_what_the_kernels_do_not_cover_is_refused_by_name(key, cfg):
    import sst_amd
    with pytest.raises(NotImplementedError, match=key):
        sst_amd.build_head(cfg)


def test_refusals_at_first_use():
    import sst_amd
    head = sst_amd.build_head(_head_cfg())
    maps = [torch.zeros(1, 18, 4, 4)], [torch.zeros(1, 42, 4, 4)], [torch.zeros(1, 12, 4, 4)]
    with pytest.raises(NotImplementedError, match='feature level'):
        head([torch.zeros(1, 8, 4, 4), torch.zeros(1, 8, 2, 2)])
    for key in ('wnms', 'wnms_gpu'):
        with pytest.raises(NotImplementedError, match=key):
            head.get_bboxes(*maps, [dict()], cfg=dict(R.TEST_CFG, **{key: True}))
    single = sst_amd.build_head(_head_cfg(train_cfg=dict(R.CASES['shipped']['train_cfg'], assigner=R.ASSIGN_3[1])))
    assert single.train_cfg['assigner']['pos_iou_thr'] == 0.5      # a single assigner dict is accepted


def test_cpu_tensors_raise():
    import sst_amd
    head = sst_amd.build_head(_head_cfg())
    boxes, labels = [torch.zeros(2, 7)], [torch.zeros(2, dtype=torch.long)]
    with pytest.raises(RuntimeError):
        sst_amd.anchor_targets(boxes, labels, (4, 4), head.anchor_generator, R.ASSIGN_3)
    with pytest.raises(RuntimeError):
        head.loss([torch.zeros(1, 18, 4, 4)], [torch.zeros(1, 42, 4, 4)], [torch.zeros(1, 12, 4, 4)], boxes, labels, [dict()])
    grid = head.anchor_generator.grid((4, 4), 'cpu')
    with pytest.raises(RuntimeError):
        sst_amd.anchor_decode(torch.zeros(18, 4, 4), torch.zeros(42, 4, 4), torch.zeros(12, 4, 4), grid, 3)
    with pytest.raises(RuntimeError):
        head.get_bboxes([torch.zeros(1, 18, 4, 4)], [torch.zeros(1, 42, 4, 4)], [torch.zeros(1, 12, 4, 4)], [dict()])
    cls, box, dirs = head([torch.zeros(1, 8, 4, 4)])           # the convolutions are torch's and run anywhere
    assert tuple(cls[0].shape) == (1, 18, 4, 4) and tuple(box[0].shape) == (1, 42, 4, 4) and tuple(dirs[0].shape) == (1, 12, 4, 4)
