"""Host side of the FSDv2 grouped sampling stage (no GPU): the torch restatement (tests/fsdv2_sample_ref.py) pinned to the
reference's own methods (tests/golden/fsdv2_sample.npz), the detectors' opt-in heads, the refusals by name and the loud failure
on CPU tensors."""
import ast
import copy
import glob
import os

import numpy as np
import pytest
import torch

import fsdv2_sample_ref as R
from conftest import GOLDEN, load_golden

V2_CONFIGS = sorted(glob.glob(os.path.join(GOLDEN, 'configs', 'fsdv2', '*.model.py')))
CASES, case_of = R.CASES, R.case_of


@pytest.fixture(scope='module')
def gold():
    return load_golden('fsdv2_sample.npz')


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
    assert [str(x) for x in gold['cases']] == CASES
    nusc = R.groups_by_names(R.NUSC_GROUPS, R.NUSC_CLASSES)
    assert case_of(gold, 'nusc')[1] == nusc == [[0], [1, 4], [3, 2], [9], [6, 5], [7, 8]]
    assert gold['nusc_seg_logits'].shape == (400, 11) and int(gold['nusc_batch']) == 2
    # rule_pair: B = 3, group 3 empty in the middle sample; group 0 too, its first point of sample 0 selected before the rule
    assert int(gold['rule_pair_batch']) == 3 and [bool(x) for x in gold['rule_pair_rule']] == [True, False, False, True, False, False]
    bidx = gold['rule_pair_batch_idx']
    assert int((bidx[gold['rule_pair_s_fg_mask_3']] == 1).sum()) == 1, 'the middle sample holds the one point the rule gave it'
    first0 = int(np.nonzero(bidx == 0)[0][0])
    data, groups, thr, _, _, _ = case_of(gold, 'rule_pair')
    assert float(R.grouped_scores(data['seg_logits'], groups)[first0, 0]) > thr[0], 'selected before the rule fired'
    # the ties: two-way and three-way in selected rows; 5e-7 below the maximum is a tie, 2e-6 is not
    for name, want in (('tie2', 2), ('tie3', 3), ('near_tie', 2)):
        data, groups, thr, extra, scale, batched = case_of(gold, name)
        masks, _ = R.group_masks(data['seg_logits'], data['batch_idx'], groups, thr, extra, batched)
        ties = torch.cat(R.centers_f64(data, groups, masks, scale)[2])
        assert int(ties.max()) == want and int((ties == want).sum()) >= 10, name
    assert gold['tie3_seg_logits'].shape[1] == 27
    data, groups, _, _, _, _ = case_of(gold, 'near_tie')
    gaps = torch.cat([(lg.max(1)[0][:, None] - lg).flatten() for lg in (data['seg_logits'][:, g] for g in groups if len(g) > 1)])
    assert bool(((gaps > 0) & (gaps < 1e-6)).any()) and bool(((gaps > 1e-6) & (gaps < 3e-6)).any())
    assert float(gold['scale_offset_scale']) == 0.3 and float(gold['nusc_offset_scale']) == 1.0
    assert np.array_equal(gold['buffer_thr32'], np.float32(np.array(R.NUSC_THRESH) + 0.05).astype(np.float64))
    assert not np.isfinite(gold['topk_thr32']).any() and [int(m.sum()) for m in gold['topk_extra']] == [40, 20, 300, 10, 5, 1]
    assert int(gold['topk_topks'][2]) > 300
    listed = set(int(c) for c in gold['unlisted_group_class'])
    assert listed < set(range(10)) and len(gold['unlisted_group_len']) == 4
    assert list(gold['one_group_group_len']) == [3]
    assert not bool(gold['unbatched_batched']) and int(gold['unbatched_batch']) == 1
    assert [bool(x) for x in gold['unbatched_rule']] == [False, False, False, True, False, False]
    assert int(gold['unbatched_s_fg_mask_3'].sum()) == 1 and bool(gold['unbatched_s_fg_mask_3'][0])
    for name in CASES:
        data, groups, thr, _, _, _ = case_of(gold, name)
        n = data['seg_logits'].size(0)
        assert 300 <= n <= 400 and n % 256 != 0
        assert bool(R.margin_ok(data['seg_logits'], groups, thr).all()), f'{name}: a grouped score is ambiguous'
        cut = int(np.nonzero(np.diff(gold[f'{name}_batch_idx']))[0][0]) + 1 if int(gold[f'{name}_batch']) > 1 else 1
        assert cut % 64 != 0, f'{name}: a wave straddles two samples'


def test_restatement_equals_the_reference(gold):
    """the grouped masks, the at-least-one rule, the voted centres, combine_classes and the projector input, case by case"""
    for name in CASES:
        data, groups, thr, extra, scale, batched = case_of(gold, name)
        smp = R.group_sample(data, groups, thr, scale, extra, batched)
        assert smp['rule'] == [bool(x) for x in gold[f'{name}_rule']], name
        for g in range(len(groups)):
            for key in ('seg_points', 'batch_idx', 'center_preds'):
                _same(smp[key][g], gold[f'{name}_s_{key}_{g}'], f'{name}: {key} of group {g}')
            _same(smp['fg_mask_list'][g], gold[f'{name}_s_fg_mask_{g}'], f'{name}: mask of group {g}')
        comb = R.combine(smp)
        rows, clipped = R.virtual_input(comb, [-51.2, -51.2, -5, 51.2, 51.2, 3])
        f = data['seg_feats'].size(1)
        _same(rows[:, f:f + 3].contiguous(), gold[f'{name}_virtual_offset'], f'{name}: the offset columns')
        _same(clipped, gold[f'{name}_clipped'], f'{name}: clipped centres')
        _same(comb['batch_idx'], gold[f'{name}_c_batch_idx'], f'{name}: combined batch_idx')
        assert bool((clipped != comb['center_preds']).any()), f'{name}: some centre is clipped'
        if name == 'nusc':
            _same(rows, gold['nusc_virtual_input'], 'nusc: the projector input')
    data, groups, _, _, _, _ = case_of(gold, 'topk')
    _same(R.topk_extra_mask(data['seg_logits'], groups, [int(x) for x in gold['topk_topks']]), gold['topk_extra'], 'top-k mask')


def test_float64_centres_bound_the_float32_ones(gold):
    """the float64 evaluation of the restatement against the reference's float64 run (which keeps its weights in float32, :858:
    one rounding of 1 / 3, an eighth of the bound), and the recorded float32 centres within the bound the GPU test uses for
    three-way ties"""
    for name in ('nusc', 'tie3'):
        data, groups, thr, extra, scale, batched = case_of(gold, name)
        masks, _ = R.group_masks(data['seg_logits'], data['batch_idx'], groups, thr, extra, batched)
        cen, bound, _ = R.centers_f64(data, groups, masks, scale)
        for g in range(len(groups)):
            ref64 = _t(gold[f'{name}_s_center_preds_f64_{g}'])
            assert bool(((cen[g] - ref64).abs() <= bound[g] / 8 + 1e-12).all()), (name, g)
            got = _t(gold[f'{name}_s_center_preds_{g}']).double()
            assert bool(((got - cen[g]).abs() <= bound[g]).all()), (name, g)


def test_second_stage_restatement(gold):
    xyz, feats, bidx, ind = (_t(gold[f'ss_pts_{k}']) for k in ('xyz', 'feats', 'batch_inds', 'indicators'))
    n_ori = int((ind == 0).sum())
    assert bool((ind[:n_ori] == 0).all()) and bool((ind[n_ori:] == 1).all()), 'the original points are the first rows'
    rng, vs = [float(x) for x in gold['ss_pc_range']], tuple(float(x) for x in gold['ss_voxel_size'])
    for with_virtual in (False, True):
        for voxel in (None, vs):
            a, b, c = R.second_stage_input(xyz, feats, bidx, ind, with_virtual, voxel, rng)
            tag = f'ss_v{int(with_virtual)}_p{int(voxel is not None)}'
            _same(a, gold[f'{tag}_xyz'], tag)
            _same(b, gold[f'{tag}_feats'], tag)
            _same(c, gold[f'{tag}_batch'], tag)
            assert bool((c[1:] >= c[:-1]).all())
    assert gold['ss_v1_p1_xyz'].shape[0] < xyz.size(0) and gold['ss_v0_p0_xyz'].shape[0] == n_ori


def _model(path):
    return ast.literal_eval(open(path).read())


@pytest.mark.parametrize('path', V2_CONFIGS, ids=[os.path.basename(p)[:-len('.model.py')] for p in V2_CONFIGS])
def test_attach_fsdv2_heads_is_opt_in(path):
    import sst_amd
    model = _model(path)
    det = sst_amd.build_detector(model)
    assert type(det) is (sst_amd.FSDV2 if model['type'] == 'FSDV2' else sst_amd.SingleStageFSDV2)
    assert not hasattr(det, 'forward_train') and not hasattr(det, 'simple_test') and not hasattr(det, 'sample')
    with pytest.raises(NotImplementedError, match='FSDV2'):
        det.attach_heads()
    keys, before = sorted(det.state_dict()), copy.deepcopy(det.unbuilt)
    assert not any(k.startswith(('bbox_head.', 'roi_head.')) for k in keys)
    assert sst_amd.attach_fsdv2_heads(det) is det
    assert det.unbuilt == before, 'unbuilt is left as it is'
    assert isinstance(det.bbox_head, sst_amd.FSDV2Head)
    plain = sst_amd.build_head(dict(before['bbox_head'], train_cfg=det.train_cfg, test_cfg=det.test_cfg))
    assert sorted(det.bbox_head.state_dict()) == sorted(plain.state_dict())
    assert [k for k in sorted(det.state_dict()) if not k.startswith(('bbox_head.', 'roi_head.'))] == keys
    if model['type'] == 'FSDV2':
        assert type(det) is sst_amd.FSDV2Step and isinstance(det, sst_amd.FSDV2)
        assert isinstance(det.roi_head, sst_amd.GroupCorrectionHead)
        assert det.roi_head.train_cfg == det.train_cfg['rcnn'] and det.roi_head.test_cfg == det.test_cfg['rcnn']
        assert any(k.startswith('roi_head.') for k in det.state_dict())
    else:
        assert type(det) is sst_amd.SingleStageFSDV2Step and not hasattr(det, 'roi_head')
    for name in ('forward_train', 'simple_test', 'sample', 'combine_classes'):
        assert callable(getattr(det, name))
    assert sst_amd.attach_fsdv2_heads(det) is det, 'a second call changes nothing'
    from sst_amd import detectors
    assert detectors.DETECTORS.get('FSDV2') is sst_amd.FSDV2 and detectors.DETECTORS.get('SingleStageFSDV2') is sst_amd.SingleStageFSDV2
    again = sst_amd.build_detector(_model(path))
    assert sorted(again.state_dict()) == keys and again.unbuilt == before and not hasattr(again, 'bbox_head')
    assert not hasattr(again, 'forward_train')


def test_refusals_by_name():
    import sst_amd
    from sst_amd import fg_group_sample as GS
    data = R.make_case(20, 11, 1, 4, 0, [[0]], [0.5])
    args = (data['seg_logits'], data['vote_offsets'], data['seg_points'], data['batch_idx'])
    with pytest.raises(NotImplementedError, match='SST_FG_MAX_CLASSES'):
        GS.group_sample_launch(torch.zeros(20, 40), torch.zeros(20, 120), data['seg_points'], data['batch_idx'],
                               [[k] for k in range(33)], [0.5] * 33, 1)
    with pytest.raises(NotImplementedError, match='SST_FG_MAX_LOGITS'):
        GS.group_sample_launch(torch.zeros(20, 65), torch.zeros(20, 195), data['seg_points'], data['batch_idx'], [[0]], [0.5], 1)
    with pytest.raises(NotImplementedError, match='listed in two groups'):
        GS.group_sample_launch(*args, [[0, 1], [2, 1]], [0.5, 0.5], 1)
    with pytest.raises(NotImplementedError, match='background'):
        GS.group_sample_launch(*args, [[0, 10]], [0.5], 1)
    with pytest.raises(NotImplementedError, match="'tram'"):
        GS.groups_by_names([['car'], ['tram']], R.NUSC_CLASSES)
    assert GS.groups_by_names(R.NUSC_GROUPS, R.NUSC_CLASSES) == R.groups_by_names(R.NUSC_GROUPS, R.NUSC_CLASSES)
    assert GS.check_groups([[0], [3, 2]], 11) == [[0], [3, 2]], 'a class that belongs to no group is legal'

    nusc = _model(os.path.join(GOLDEN, 'configs', 'fsdv2', 'fsdv2_nusc_1x.model.py'))
    det = sst_amd.attach_fsdv2_heads(sst_amd.build_detector(copy.deepcopy(nusc)))
    with pytest.raises(NotImplementedError, match='group_sample needs seg_logits'):
        det.sample(dict(data, seg_logits=torch.zeros(20, 10)), data['vote_offsets'])
    det.train()
    det.train_cfg = dict(det.train_cfg, add_gt_fg_points=True, disable_pretrain=False)
    with pytest.raises(NotImplementedError, match='add_gt_fg_points'):
        det.sample(dict(data), data['vote_offsets'], batch_size=1)
    with pytest.raises(NotImplementedError, match='aug_test'):
        det.aug_test(None, None)
    with pytest.raises(NotImplementedError, match='seg_logits='):
        det.get_fg_mask(None, None, 0, None, None, None)
    waymo = _model(os.path.join(GOLDEN, 'configs', 'fsdv2', 'fsdv2_waymo_1x.model.py'))
    det_w = sst_amd.attach_fsdv2_heads(sst_amd.build_detector(copy.deepcopy(waymo)))
    with pytest.raises(NotImplementedError, match='fits neither'):
        det_w.sample(dict(data, seg_logits=torch.zeros(20, 5)), data['vote_offsets'])
    for key, value, match in (('centroid_alpha', 0.5, 'centroid_alpha'), ('offset_weight', 'softmax', 'offset_weight')):
        bad = copy.deepcopy(nusc)
        bad['train_cfg'][key] = value
        with pytest.raises(NotImplementedError, match=match):
            sst_amd.attach_fsdv2_heads(sst_amd.build_detector(bad))
    bad = copy.deepcopy(nusc)
    bad['train_cfg']['baseline_mode'] = True
    with pytest.raises(NotImplementedError, match='baseline_mode'):
        sst_amd.build_detector(bad)
    fsd = _model(os.path.join(GOLDEN, 'configs', 'fsd', 'fsd_waymoD1_1x.model.py'))
    with pytest.raises(NotImplementedError, match='not an FSDv2 detector'):
        sst_amd.attach_fsdv2_heads(sst_amd.build_detector(fsd))


def test_cpu_tensors_fail_loudly():
    from sst_amd import fg_group_sample as GS
    groups, thr = R.groups_by_names(R.NUSC_GROUPS, R.NUSC_CLASSES), R.thresholds32(R.NUSC_THRESH)
    data = R.make_case(50, 11, 2, 8, 1, groups, thr)
    with pytest.raises(RuntimeError, match='CUDA/HIP'):
        GS.group_sample(data['seg_logits'], data['vote_offsets'], data['seg_points'], data['batch_idx'], groups, thr, 2)
    with pytest.raises(RuntimeError, match='CUDA/HIP'):
        GS.group_topk_extra_mask(data['seg_logits'], groups, [5] * 6)
    fake = dict(slot=torch.zeros((6, 50), dtype=torch.int32), src_cat=torch.zeros(0, dtype=torch.int32), center_cat=torch.zeros(0, 3),
                class_offsets=[0] * 7)
    with pytest.raises(RuntimeError, match='CUDA/HIP'):
        GS.virtual_rows(fake, data['seg_feats'], data['seg_logits'], data['seg_points'], [-51.2, -51.2, -5, 51.2, 51.2, 3])
    lo, hi = GS.clip_bounds([-51.2, -51.2, -5, 51.2, 51.2, 3])
    rlo, rhi = R.clip_bounds([-51.2, -51.2, -5, 51.2, 51.2, 3])
    assert lo == rlo.tolist() and hi == rhi.tolist()
    assert lo == [float(np.float32(v + 1e-5)) for v in (-51.2, -51.2, -5)], 'the bounds of the reference (formed in double)'


def test_virtual_input_branch_is_additive():
    """VirtualVoxelExtractor.extract_feat reads 'virtual_input' only when the key is there"""
    import inspect
    from sst_amd.virtual_voxel import VirtualVoxelExtractor
    src = inspect.getsource(VirtualVoxelExtractor.extract_feat)
    assert "'virtual_input' in sampled_dict" in src and 'self.clip_points(' in src
