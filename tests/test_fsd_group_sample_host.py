"""Host: the torch restatement of ``SingleStageFSD.group_sample`` (tests/fsd_group_sample_ref.py) against the reference's own
methods (tests/golden/fsd_group_sample.npz, tests/golden/make_fsd_group_sample.py): masks, rule flags, row orders and lists
are equal, the voted centres bit for bit in float32, the grouped scores and offset weights too."""
import numpy as np
import pytest
import torch

import fsd_group_sample_ref as R
from conftest import load_golden


@pytest.fixture(scope='module')
def gold():
    return load_golden('fsd_group_sample.npz')


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def case_of(gold, name):
    """-> (data, layout name, groups, float32 thresholds, extra mask or None)"""
    layout = str(gold[f'{name}_layout'])
    data = {k: _t(gold[f'{name}_{k}']) for k in R.KEYS}
    groups = R.layout(layout)[2]
    thr = [float(x) for x in gold[f'{name}_thr32']]
    extra = None
    if f'{name}_topks' in gold:
        extra = R.topk_extra_mask(data['seg_logits'], groups, [int(x) for x in gold[f'{name}_topks']])
    return data, layout, groups, thr, extra


def cases(gold):
    return [str(c) for c in gold['cases']]


def test_the_golden_holds_the_cases_the_issue_names(gold):
    names = cases(gold)
    for layout in ('argo2', 'small'):
        assert {f'{layout}_b1', f'{layout}_b2', f'{layout}_b3', f'{layout}_rule', f'{layout}_rule_all', f'{layout}_tie2',
                f'{layout}_buffer', f'{layout}_topk'} <= set(names)
        assert [int(gold[f'{layout}_b{b}_batch']) for b in (1, 2, 3)] == [1, 2, 3]
        assert gold[f'{layout}_rule_rule'].tolist()[-1] is True and not all(gold[f'{layout}_rule_rule'].tolist())
        assert all(gold[f'{layout}_rule_all_rule'].tolist())
    assert gold['argo2_b2_seg_logits'].shape[1] == 27 and gold['small_b2_seg_logits'].shape[1] == 4
    weights = np.concatenate([gold[f'argo2_tie2_s_weight_{g}'].reshape(-1) for g in range(1, 5)], 0)
    assert (weights == 0.5).any() and set(np.unique(weights)) <= {0.0, 0.5, 1.0}
    for name in names:                                   # nothing is ambiguous: the margins hold for every stored row
        data, _, groups, thr, _ = case_of(gold, name)
        assert bool(R.margin_ok(data['seg_logits'], groups, thr).all()), name


def test_restatement_equals_the_reference(gold):
    for name in cases(gold):
        data, layout, groups, thr, extra = case_of(gold, name)
        classes, group_names = R.layout(layout)[:2]
        ref = R.group_sample(data, groups, thr, extra)
        assert ref['rule'] == [bool(x) for x in gold[f'{name}_rule']], name
        scores = R.gather_group_by_names(data['seg_logits'].softmax(1)[:, :-1], group_names, classes)
        assert torch.equal(scores, _t(gold[f'{name}_grouped_scores'])), name
        for g in range(len(groups)):
            mask = ref['fg_mask_list'][g]
            assert torch.equal(mask, _t(gold[f'{name}_s_fg_mask_{g}'])), (name, g)
            for key in ('seg_points', 'batch_idx'):
                assert torch.equal(ref[key][g], _t(gold[f'{name}_s_{key}_{g}'])), (name, key, g)
            got, want = ref['center_preds'][g], _t(gold[f'{name}_s_center_preds_{g}'])
            assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f'{name}: centres of group {g} not bit for bit'
            w = R.get_offset_weight(data['seg_logits'][:, groups[g]][mask])
            assert torch.equal(w, _t(gold[f'{name}_s_weight_{g}'])), (name, g)


def test_detector_methods_equal_the_reference_on_the_host(gold):
    """gather_group_by_names, gather_group and get_offset_weight of sst_amd's SingleStageFSD are plain tensor code"""
    from sst_amd.detectors import SingleStageFSD
    det = SingleStageFSD.__new__(SingleStageFSD)
    torch.nn.Module.__init__(det)
    classes, group_names, groups, _ = R.layout('argo2')
    det.cfg = det.train_cfg = det.test_cfg = dict(group_names=group_names, class_names=classes, offset_weight='max')
    logits = _t(gold['argo2_tie2_seg_logits'])
    scores = logits.softmax(1)[:, :-1]
    assert torch.equal(det.gather_group_by_names(scores), _t(gold['argo2_tie2_grouped_scores']))
    assert torch.allclose(det.gather_group(scores, [len(g) for g in group_names]), det.gather_group_by_names(scores), atol=0, rtol=0)
    for g in range(6):
        mask = _t(gold[f'argo2_tie2_s_fg_mask_{g}'])
        assert torch.equal(det.get_offset_weight(logits[:, groups[g]][mask]), _t(gold[f'argo2_tie2_s_weight_{g}']))
