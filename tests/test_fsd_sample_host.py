"""Host side of the FSD foreground sampling stage (no GPU): the torch restatement (tests/fsd_sample_ref.py) pinned to the
reference's own methods (tests/golden/fsd_sample.npz), the detectors' opt-in heads, the refusals by name and the loud failure
on CPU tensors."""
import ast
import copy
import glob
import os

import numpy as np
import pytest
import torch

import fsd_sample_ref as R
from conftest import GOLDEN, load_golden

KEYS = ('seg_points', 'seg_logits', 'seg_vote_preds', 'seg_feats', 'batch_idx', 'vote_offsets')
FSD_CONFIGS = sorted(glob.glob(os.path.join(GOLDEN, 'configs', 'fsd', '*.model.py')))


@pytest.fixture(scope='module')
def gold():
    return load_golden('fsd_sample.npz')


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _same(a, b, what):
    b = _t(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f'{what}: {a.dtype} {tuple(a.shape)} vs {b.dtype} {tuple(b.shape)}'
    if a.is_floating_point():
        assert torch.equal(a.contiguous().view(torch.int32), b.view(torch.int32)), f'{what}: not bit for bit'
    else:
        assert torch.equal(a, b), what


def test_cases_cover_the_issue(gold):
    names = [str(x) for x in gold['cases']]
    assert names == ['plain', 'rule_pair', 'buffer', 'topk', 'gt_points', 'class_none', 'class_all', 'single']
    assert [bool(x) for x in gold['rule_pair_rule']] == [True, False, False]
    first0 = int(np.nonzero(gold['rule_pair_batch_idx'] == 0)[0][0])
    assert gold['rule_pair_seg_logits'][first0, 0] > 0, 'the first point of sample 0 was selected before the rule fired'
    assert [bool(x) for x in gold['class_none_rule']] == [False, True, False] and int(gold['class_none_s_fg_mask_1'].sum()) == 2
    assert bool(gold['class_all_s_fg_mask_2'].all())
    assert not np.isfinite(gold['topk_thr32']).any() and [int(gold['topk_extra'][k].sum()) for k in range(3)] == [40, 20, 300]
    assert np.allclose(gold['buffer_thr32'], np.float32(np.array([0.5, 0.3, 0.6]) + 0.1), rtol=0, atol=0)
    assert gold['single_seg_logits'].shape[1] == 1 and gold['plain_seg_feats'].shape[1] == 67
    for name in names:
        assert not gold[f'{name}_valid_0'].all(), f'{name}: the valid-mask step removes rows'
        assert bool(R.margin_ok(_t(gold[f'{name}_seg_logits']), list(gold[f'{name}_thr32'])).all())


def test_restatement_equals_the_reference(gold):
    """sample, the at-least-one rule, update_sample_results_by_mask, combine_classes and both prepare_*_roi_input"""
    for name in (str(x) for x in gold['cases']):
        data = {k: _t(gold[f'{name}_{k}']) for k in KEYS}
        thr = [float(x) for x in gold[f'{name}_thr32']]
        extra = _t(gold[f'{name}_extra']) if f'{name}_extra' in gold else None
        c = data['seg_logits'].size(1)
        smp = R.sample(data, thr, extra)
        assert smp['rule'] == [bool(x) for x in gold[f'{name}_rule']], name
        for k in range(c):
            for key in ('seg_points', 'batch_idx', 'center_preds'):
                _same(smp[key][k], gold[f'{name}_s_{key}_{k}'], f'{name}: {key} of class {k}')
            _same(smp['fg_mask_list'][k], gold[f'{name}_s_fg_mask_{k}'], f'{name}: mask of class {k}')
        valid = [_t(gold[f'{name}_valid_{k}']) for k in range(c)]
        upd = R.update_by_mask(smp, valid)
        comb = R.combine(upd)
        _same(comb['pts_feats'], gold[f'{name}_pts_feats'], f'{name}: pts_feats')
        _same(comb['points'], gold[f'{name}_points'], f'{name}: points')
        _same(comb['center_preds'], gold[f'{name}_center_preds'], f'{name}: center_preds')
        for k in range(c):
            _same(upd['fg_mask_list'][k], gold[f'{name}_final_mask_{k}'], f'{name}: final mask of class {k}')
        cluster = _t(gold[f'{name}_cluster_pts_feats'])
        prepare = R.roi_single if c == 1 else R.roi_multi
        pts, feats, bidx = prepare(data['seg_points'], cluster, data['seg_feats'], upd['fg_mask_list'], data['batch_idx'])
        _same(pts, gold[f'{name}_roi_points'], f'{name}: roi points')
        _same(feats, gold[f'{name}_roi_feats'], f'{name}: roi cat_feats')
        _same(bidx, gold[f'{name}_roi_batch'], f'{name}: roi batch inds')
    # top-k indices as the reference sets them; the float32 centre is the rounded float64 one (one add)
    _same(R.topk_extra_mask(_t(gold['topk_seg_logits']), [40, 20, 400]), gold['topk_extra'], 'top-k mask')
    for k in range(3):
        assert np.array_equal(gold[f'plain_s_center_preds_{k}'], gold[f'plain_s_center_preds_f64_{k}'].astype(np.float32))


def test_pre_voxelize_golden_is_a_segmented_mean(gold):
    """new_coors / inverse = torch.unique(dim=0) of (sample, z, y, x); the features are the group means (1e-5: the bar for
    segmented means) - what SingleStageFSD.pre_voxelize is compared with on the GPU"""
    pts, bidx = _t(gold['pv_in_seg_points']), _t(gold['pv_in_batch_idx'])
    lo = torch.tensor(gold['pv_pc_range'][:3], dtype=torch.float32)
    coors = torch.div(pts[:, :3] - lo[None], torch.tensor([0.5, 0.5, 0.5])[None], rounding_mode='floor').long()[:, [2, 1, 0]]
    new_coors, inv = torch.unique(torch.cat([bidx[:, None], coors], 1), return_inverse=True, dim=0)
    assert np.array_equal(new_coors.numpy(), gold['pv_new_coors']) and np.array_equal(inv.numpy(), gold['pv_unq_inv'])
    assert np.array_equal(gold['pv_out_batch_idx'], gold['pv_new_coors'][:, 0])
    for k in ('seg_points', 'seg_feats'):
        assert np.abs(gold[f'pv_out_{k}'] - gold[f'pv_out_f64_{k}']).max() < 1e-5


def _model(path):
    return ast.literal_eval(open(path).read())


@pytest.mark.parametrize('path', FSD_CONFIGS, ids=[os.path.basename(p)[:-len('.model.py')] for p in FSD_CONFIGS])
def test_attach_heads_is_opt_in(path):
    import sst_amd
    model = _model(path)
    det = sst_amd.build_detector(model)
    if model['type'] not in ('FSD', 'SingleStageFSD'):
        assert not hasattr(det, 'attach_heads')          # the pre-training config is the segmentor alone
        return
    keys, before = sorted(det.state_dict()), copy.deepcopy(det.unbuilt)
    assert not any(k.startswith(('bbox_head.', 'roi_head.')) for k in keys) and set(before) >= {'bbox_head'}
    with pytest.raises(RuntimeError, match=r'attach_heads\(\)'):
        det.forward_train([torch.zeros(4, 5)], [{}], [torch.zeros(0, 7)], [torch.zeros(0, dtype=torch.long)])
    with pytest.raises(RuntimeError, match=r'attach_heads\(\)'):
        det.simple_test([torch.zeros(4, 5)], [{}])
    assert det.attach_heads() is det
    assert det.unbuilt == before, 'unbuilt is left as it is'
    assert isinstance(det.bbox_head, sst_amd.SparseClusterHeadV2)
    plain = sst_amd.build_head(dict(before['bbox_head'], train_cfg=det.train_cfg, test_cfg=det.test_cfg))
    assert sorted(det.bbox_head.state_dict()) == sorted(plain.state_dict())
    new_keys = sorted(det.state_dict())
    assert [k for k in new_keys if not k.startswith(('bbox_head.', 'roi_head.'))] == keys
    if model['type'] == 'FSD':
        assert isinstance(det.roi_head, sst_amd.GroupCorrectionHead)
        assert det.roi_head.train_cfg == det.train_cfg['rcnn'] and det.roi_head.test_cfg == det.test_cfg['rcnn']
    # a second detector built without the call is what it was
    again = sst_amd.build_detector(_model(path))
    assert sorted(again.state_dict()) == keys and again.unbuilt == before and not hasattr(again, 'bbox_head')


def test_refusals_by_name():
    import sst_amd
    from sst_amd import fg_sample as FS
    model = _model(os.path.join(GOLDEN, 'configs', 'fsd', 'fsd_waymoD1_1x.model.py'))
    det = sst_amd.build_detector(model).attach_heads()
    data, _ = R.make_case(20, 3, 1, 4, seed=0)
    det.cfg = dict(det.cfg, group_sample=True)
    with pytest.raises(NotImplementedError, match='group_sample'):
        det.sample(data, data['vote_offsets'])
    det.cfg = dict(det.cfg, group_sample=False)
    wide = dict(data, seg_logits=torch.zeros(20, 4))
    with pytest.raises(NotImplementedError, match='softmax'):
        det.sample(wide, data['vote_offsets'])
    with pytest.raises(NotImplementedError, match='seg_logits'):
        det.get_fg_mask(data['seg_logits'].sigmoid(), data['seg_points'][:, :3], 0, data['batch_idx'], None, None)
    with pytest.raises(NotImplementedError, match='SST_FG_MAX_CLASSES'):
        FS.fg_sample_launch(None, None, data['seg_points'], data['batch_idx'], [0.5] * 33, 1)
    v2 = copy.deepcopy(model)
    v2['bbox_head']['type'] = 'FSDV2Head'
    det2 = sst_amd.build_detector(v2)
    with pytest.raises(NotImplementedError, match='FSDV2Head'):
        det2.attach_heads()
    # FSDv2 is out of scope: its detectors refuse by the name of their head
    for path in sorted(glob.glob(os.path.join(GOLDEN, 'configs', 'fsdv2', '*.model.py')))[:1]:
        det3 = sst_amd.build_detector(_model(path))
        with pytest.raises(NotImplementedError, match='FSDV2'):
            det3.attach_heads()
        assert not hasattr(det3, 'forward_train'), 'no FSDv2 training step is offered'


def test_cpu_tensors_fail_loudly():
    from sst_amd import fg_sample as FS
    data, thr = R.make_case(50, 3, 2, 8, seed=1)
    with pytest.raises(RuntimeError, match='CUDA/HIP'):
        FS.fg_sample(data['seg_logits'], data['vote_offsets'], data['seg_points'], data['batch_idx'], thr, 2)
    masks, _ = R.fg_masks(data['seg_logits'], data['batch_idx'], thr)
    with pytest.raises(RuntimeError, match='CUDA/HIP'):
        FS.roi_input(data['seg_points'], torch.zeros(int(masks.sum()), 5), data['seg_feats'], list(masks), data['batch_idx'], 2)
    with pytest.raises(RuntimeError, match='CUDA/HIP'):
        FS.roi_input_single(data['seg_points'], torch.zeros(int(masks[0].sum()), 5), data['seg_feats'], [masks[0]], data['batch_idx'])
    fake = dict(slot=torch.zeros((3, 50), dtype=torch.int32), src=[torch.zeros(0, dtype=torch.int32)] * 3,
                center_preds=[torch.zeros(0, 3)] * 3)
    with pytest.raises(RuntimeError, match='CUDA/HIP'):
        FS.fg_gather_cat(fake, [torch.zeros(0, dtype=torch.long)] * 3, data['seg_logits'], data['seg_vote_preds'],
                         data['seg_feats'], data['seg_points'])
    assert FS.round_thresholds([0.3], 0.1) == [float(np.float32(0.3 + 0.1))] == R.thresholds32([0.3], 0.1)
