"""CenterHead's targets, losses and decoding without a GPU: the restatement of tests/center_head_ref.py against the reference's
own methods (tests/golden/center_head_train.npz), the construction of CenterHead from the shipped configs, and the loud
failures of the Python entry points on CPU tensors."""
import ast
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

import center_head_ref as R

CONFIGS = ('sst_waymoD5_1x_3class_centerhead', 'sst_waymoD1_2x_3class_centerhead')


@pytest.fixture(scope='module')
def gold():
    return load_golden('center_head_train.npz')


def scene(gold, case):
    cols = R.CASES[case][3]
    return [gold[f'boxes{s}'][:, :cols] for s in range(3)], [gold[f'labels{s}'] for s in range(3)]


def restated_targets(gold, case):
    cfg, tasks, norm_bbox, _ = R.CASES[case]
    boxes, labels = scene(gold, case)
    return R.targets(boxes, labels, tasks, cfg, norm_bbox)


@pytest.mark.parametrize('case', list(R.CASES))
def test_restated_targets_equal_the_reference(gold, case):
    hm, anno, ind, mask = restated_targets(gold, case)
    for t in range(len(R.CASES[case][1])):
        g_hm, g_anno = gold[f'tgt_{case}_t{t}_heatmap'], gold[f'tgt_{case}_t{t}_anno']
        assert np.array_equal(ind[t], gold[f'tgt_{case}_t{t}_ind'])
        assert np.array_equal(mask[t], gold[f'tgt_{case}_t{t}_mask'])
        assert hm[t].shape == g_hm.shape == (3, len(R.CASES[case][1][t]['class_names']), R.H, R.W)
        assert np.array_equal(hm[t] == 0, g_hm == 0) and np.array_equal(hm[t] == 1, g_hm == 1)
        assert np.array_equal(hm[t], g_hm)                                   # numpy's exp on both sides
        assert np.array_equal(anno[t][..., [0, 1, 2, 8, 9]], g_anno[..., [0, 1, 2, 8, 9]])
        # log / sin / cos: torch's CPU functions on a whole array here, on single boxes in the reference
        assert R.ulp_distance(anno[t][..., 3:8], g_anno[..., 3:8]).max() <= 1


def test_the_scene_holds_the_cases_the_targets_must_get_right(gold):
    """what the fixture was built to contain, read back from the reference's outputs"""
    hm, anno, ind, mask = (gold[f'tgt_shipped_t0_{k}'] for k in ('heatmap', 'anno', 'ind', 'mask'))
    labels = gold['labels0']
    assert len(gold['boxes1']) == 0 and mask[1].sum() == 0 and not hm[1].any()
    assert (labels == -1).sum() == 2
    m0 = mask[0].astype(bool)
    n_task = int((labels >= 0).sum())
    assert m0[:n_task].sum() == n_task - 2 and not m0[n_task:].any()       # the zero-width box and the one outside keep a slot
    cells, count = np.unique(ind[0][m0], return_counts=True)
    assert (count == 2).sum() >= 2                                          # one class / two classes in one cell
    xs, ys = ind[0][m0] % R.W, ind[0][m0] // R.W
    assert xs.min() == 0 and xs.max() == R.W - 1 and ys.min() == 0 and ys.max() == R.H - 1
    assert (anno[0][m0][:, 0] < 0).sum() == 1                               # the centre with coor_x in (-1, 0) sits in cell 0
    # class-grouped slots: the truncated case keeps the first 8 of the same list
    m8, i8 = gold['tgt_max8_t0_mask'], gold['tgt_max8_t0_ind']
    assert m8.shape == (3, 8) and np.array_equal(i8, ind[:, :8]) and np.array_equal(m8, mask[:, :8])
    # two tasks split the one-task list by class
    two = [gold[f'tgt_two_tasks_t{t}_mask'] for t in range(2)]
    assert two[0].sum() + two[1].sum() == mask.sum()
    # osf 2 on half the voxel size is the same map
    assert np.array_equal(gold['tgt_osf2_t0_ind'], ind)


def test_min_radius_decides_for_small_boxes(gold):
    cfg = R.CASES['shipped'][0]
    vs = np.float32(cfg['voxel_size'][0])
    radii = [int(R.gaussian_radius(np.float32(b[4]) / vs, np.float32(b[3]) / vs, cfg['gaussian_overlap']))
             for b in gold['boxes0'] if b[3] > 0]
    assert min(radii) < cfg['min_radius'] < max(radii)


@pytest.mark.parametrize('case', R.LOSS_CASES)
def test_restated_losses_equal_the_reference(gold, case):
    cfg, tasks, _, _ = R.CASES[case]
    hm, anno, ind, mask = restated_targets(gold, case)
    heads = R.split_heads(gold['head_maps'].astype(np.float32))
    at = 0
    for t, task in enumerate(tasks):
        c = len(task['class_names'])
        logits = gold['logits'][:, at:at + c]
        at += c
        got = R.losses_and_grads(logits, heads, gold[f'tgt_{case}_t{t}_heatmap'], gold[f'tgt_{case}_t{t}_anno'], ind[t], mask[t],
                                 cfg['code_weights'], R.W_CLS, R.W_BBOX)
        pre = f'loss_{case}_t{t}_f64_'
        assert abs(got['loss_heatmap'] - gold[pre + 'loss_heatmap']) <= 1e-12 * abs(gold[pre + 'loss_heatmap'])
        assert abs(got['loss_bbox'] - gold[pre + 'loss_bbox']) <= 1e-12 * abs(gold[pre + 'loss_bbox'])
        d_logits = np.zeros_like(gold['logits'], dtype=np.float64)
        d_logits[:, at - c:at] = got['d_logits']
        ref8 = gold[pre + 'd_logits_8th']
        assert np.abs(d_logits.reshape(-1)[::8] - ref8).max() <= 1e-12 * np.abs(ref8).max()
        assert abs(np.abs(got['d_logits']).sum() - gold[pre + 'd_logits_abs']) <= 1e-11 * gold[pre + 'd_logits_abs']
        d_heads = np.concatenate(got['d_heads'], 1)
        ref = gold[pre + 'd_heads']
        assert np.array_equal(d_heads != 0, ref != 0)
        assert np.abs(d_heads - ref).max() <= 1e-12 * np.abs(ref).max()
        for k in ('loss_heatmap', 'loss_bbox', 'd_logits', 'd_heads'):
            assert 0 <= float(gold[f'noise_{case}_t{t}_{k}']) < 1e-5


def test_loss_inputs_reach_past_both_clamp_bounds(gold):
    z = gold['logits']
    assert (z > 9.3).sum() >= 20 and (z < -9.3).sum() >= 20
    assert (np.abs(np.abs(z) - 9.21024) > 1e-3).all()


@pytest.mark.parametrize('case', list(R.DECODE_CASES))
def test_restated_decode_equals_the_reference(gold, case):
    with_vel, norm_bbox = R.DECODE_CASES[case], R.CASES[case][2]
    reg, hei, dim, rot, vel = R.split_heads(gold['head_maps'].astype(np.float32))
    coder = R.coder_cfg(case, float(gold['decode_score_threshold']))
    boxes, scores, labels, keep = R.decode(R.heat_of(gold['logits']), reg, hei, dim, rot, vel if with_vel else None, coder,
                                           norm_bbox)
    assert boxes.shape == (3, R.MAX_NUM, 9 if with_vel else 7)
    for i in range(3):
        g_boxes, g_scores = gold[f'decode_{case}_s{i}_bboxes'], gold[f'decode_{case}_s{i}_scores']
        assert 0 < len(g_scores) < R.MAX_NUM
        assert np.array_equal(scores[i][keep[i]], g_scores)
        assert np.array_equal(labels[i][keep[i]].astype(np.float32), gold[f'decode_{case}_s{i}_labels'])
        plain = [0, 1, 2] + ([7, 8] if with_vel else []) + ([] if norm_bbox else [3, 4, 5])
        assert np.array_equal(boxes[i][keep[i]][:, plain], g_boxes[:, plain])
        assert R.ulp_distance(boxes[i][keep[i]], g_boxes).max() <= 1        # exp / atan2 on other array shapes


def _model_cfg(name):
    path = os.path.join(GOLDEN, 'configs', 'sst_refactor', name + '.model.py')
    return ast.literal_eval(open(path).read())


@pytest.mark.parametrize('name', CONFIGS)
def test_center_head_constructs_from_the_shipped_configs(name):
    import sst_amd
    model = _model_cfg(name)
    cfg = dict(model['bbox_head'], train_cfg=model['train_cfg'], test_cfg=model['test_cfg'])
    head = sst_amd.build_head(cfg)
    assert isinstance(head, sst_amd.CenterHead) and isinstance(head.bbox_coder, sst_amd.CenterPointBBoxCoder)
    assert head.num_classes == [3] and head.norm_bbox is True and not head.loss_unbuilt
    assert head.loss_weight_bbox == 2.0 and head.loss_weight_cls == 1.0
    assert head.bbox_coder.max_num == 4096 and head.bbox_coder.code_size == 9
    for key in ('in_channels', 'share_conv_channel', 'separate_head', 'common_heads', 'norm_cfg'):
        assert head.unbuilt[key] == model['bbox_head'][key]
    assert not list(head.parameters())
    with pytest.raises(NotImplementedError, match='DCNSeparateHead'):
        head(torch.zeros(1, 128, 4, 4))
    # the detector keeps parking the head's config, exactly as before
    det = sst_amd.build_detector(model)
    assert det.unbuilt['bbox_head'] == model['bbox_head']
    # circle NMS is refused by name
    head.test_cfg = dict(head.test_cfg, nms_type='circle')
    with pytest.raises(NotImplementedError, match='circle'):
        head.get_bboxes([[dict()]], [dict()])


def test_ops_raise_on_cpu_tensors(gold):
    import sst_amd
    cfg, tasks, norm_bbox, _ = R.CASES['shipped']
    boxes, labels = scene(gold, 'shipped')
    with pytest.raises(RuntimeError):
        sst_amd.center_targets([torch.from_numpy(b) for b in boxes], [torch.from_numpy(l) for l in labels], tasks, cfg, norm_bbox)
    heads = [torch.from_numpy(h) for h in R.split_heads(gold['head_maps'].astype(np.float32))]
    logits = torch.from_numpy(gold['logits'])
    tgt = [torch.from_numpy(gold[f'tgt_shipped_t0_{k}']) for k in ('heatmap', 'anno', 'ind', 'mask')]
    with pytest.raises(RuntimeError):
        sst_amd.center_loss(logits, *heads, *tgt, cfg['code_weights'])
    reg, hei, dim, rot, vel = heads
    inds = torch.zeros((3, 4), dtype=torch.long)
    with pytest.raises(RuntimeError):
        sst_amd.center_decode(inds, torch.zeros(3, 4), reg, hei, dim, rot[:, 0:1], rot[:, 1:2], vel, 1, (0.32, 0.32), R.PC[:2])
    coder = sst_amd.CenterPointBBoxCoder(**R.coder_cfg('shipped', 0.1))
    with pytest.raises(RuntimeError):
        coder.decode(torch.rand(3, 3, R.H, R.W), rot[:, 0:1], rot[:, 1:2], hei, dim, vel, reg=reg)
    head = sst_amd.CenterHead(tasks=tasks, train_cfg=cfg, test_cfg=dict(nms_type='rotate'),
                              bbox_coder=dict(type='CenterPointBBoxCoder', **R.coder_cfg('shipped', 0.1)))
    with pytest.raises(RuntimeError):
        head.get_targets([torch.from_numpy(b) for b in boxes], [torch.from_numpy(l) for l in labels])
