"""GPU: ``SingleStageFSD.sample`` with ``group_sample`` (the softmax score path over csrc/fg_group_sample.hip) against the
reference's own methods (tests/golden/fsd_group_sample.npz) and against the torch restatement
(tests/fsd_group_sample_ref.py) on the device: masks, slots, sources, counts and copied rows are equal and the centres bit for
bit (rows hold at most two equal maxima, so the weights 1 and 0.5 make every product exact; only the rows the rule picks in
the every-group-empty case tie more widely, and those stay within seven float32 roundings of the float64 value); after
``update_sample_results_by_mask`` the combined rows equal boolean indexing and their gradient is bit-equal on integer data.
Every grouped score is (K + 8) * 2^-23 clear of its threshold (asserted), so the masks do not depend on whose exp ran."""
import numpy as np
import pytest
import torch

import fsd_group_sample_ref as R
from conftest import load_golden
from test_fsd_group_sample_host import case_of, cases
from test_gpu_fg_group_sample import _bits, _check

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def gold():
    return load_golden('fsd_group_sample.npz')


def detector(layout, training=False, runtime_info=None, **cfg):
    """a SingleStageFSD with the attributes the sampling stage reads (no network is built)"""
    from sst_amd.detectors import SingleStageFSD
    classes, group_names, _, _ = R.layout(layout)
    det = SingleStageFSD.__new__(SingleStageFSD)
    torch.nn.Module.__init__(det)
    det.num_classes = len(classes)
    det.train_cfg = det.test_cfg = det.cfg = dict(score_thresh=R.LAYOUTS[layout][2], group_names=group_names, class_names=classes,
                                                  group_sample=True, offset_weight='max', **cfg)
    det.runtime_info = runtime_info if runtime_info is not None else {}
    det.print_info = {}
    det.train(training)
    return det


def run(det, data, batch):
    d = {k: v.to(DEV) for k, v in data.items()}
    return d, det.sample(d, d['vote_offsets'], batch_size=batch)


def after_the_cluster_filter(det, d, out, ref, seed):
    """drawn valid masks per group -> the detector's combined rows against boolean indexing, forward and gradient"""
    g = torch.Generator().manual_seed(seed)
    valid = [(torch.rand(m.size(0), generator=g) < 0.7).to(DEV) for m in ref['seg_points']]
    feats = d['seg_feats'].clone().requires_grad_(True)
    src = dict(out['source'], seg_feats=feats)
    upd = det.update_sample_results_by_mask(dict(out, source=src), valid)
    comb = det.combine_classes(upd, ['seg_points', 'pts_feats', 'center_preds'])
    feats2 = d['seg_feats'].clone().requires_grad_(True)
    want = R.combine(R.update_by_mask({k: v for k, v in dict(ref, seg_feats=[feats2[m] for m in ref['fg_mask_list']]).items()},
                                      valid))
    _bits(comb['seg_points'], want['points'], 'combined points')
    _bits(comb['pts_feats'].detach(), want['pts_feats'].detach(), 'combined rows')
    _bits(comb['center_preds'], want['center_preds'], 'combined centres')
    for a, b in zip(upd['fg_mask_list'], R.update_by_mask(ref, valid)['fg_mask_list']):
        _bits(a, b, 'final masks')
    w = torch.randint(-3, 4, comb['pts_feats'].shape, generator=g).float().to(DEV)       # integer data: any summation order agrees
    (comb['pts_feats'] * w).sum().backward()
    (want['pts_feats'] * w).sum().backward()
    _bits(feats.grad, feats2.grad, 'gradient of seg_feats')


@pytest.mark.parametrize('name', ['argo2_b1', 'argo2_b2', 'argo2_b3', 'argo2_rule', 'argo2_rule_all', 'argo2_tie2', 'argo2_buffer',
                                  'argo2_topk', 'small_b1', 'small_b2', 'small_b3', 'small_rule', 'small_rule_all', 'small_tie2',
                                  'small_buffer', 'small_topk'])
def test_sample_equals_the_reference(gold, name):
    assert name in cases(gold)
    data, layout, groups, thr, extra = case_of(gold, name)
    kw = {}
    if name.endswith('_buffer'):
        kw = dict(training=True, runtime_info=dict(threshold_buffer=0.1, enable_detection=True))
    elif name.endswith('_topk'):
        kw = dict(training=True, runtime_info={}, disable_pretrain=True, disable_pretrain_topks=[int(x) for x in gold[f'{name}_topks']])
    det = detector(layout, **kw)
    d, out = run(det, data, int(gold[f'{name}_batch']))
    ref = dict(fg_mask_list=[torch.from_numpy(gold[f'{name}_s_fg_mask_{g}']) for g in range(len(groups))],
               rule=[bool(x) for x in gold[f'{name}_rule']])
    for key in ('seg_points', 'batch_idx', 'center_preds'):
        ref[key] = [torch.from_numpy(np.ascontiguousarray(gold[f'{name}_s_{key}_{g}'])) for g in range(len(groups))]
    _check(d, out, ref, groups, 1, name)
    if not name.endswith('_rule_all'):   # there the rule picks rows whose foreground logits are all -30: up to nine equal maxima,
        # which _check holds to the float64 evaluation within seven roundings; everywhere else every centre is compared bit for bit
        assert int(torch.cat(R.centers_f64(d, groups, [m.to(DEV) for m in ref['fg_mask_list']], 1)[2]).max()) <= 2
    on_dev = R.group_sample(d, groups, thr, None if extra is None else extra.to(DEV))
    _check(d, out, on_dev, groups, 1, f'{name} (device restatement)')
    assert out['source'] is d or set(out['source']) == set(d)
    after_the_cluster_filter(det, d, out, on_dev, seed=len(name))


@pytest.mark.parametrize('layout', ['argo2', 'small'])
@pytest.mark.parametrize('b', [1, 2, 3])
@pytest.mark.parametrize('n', [1, 255, 256, 257, 1000])
def test_sizes_at_the_block_edges(n, b, layout):
    groups, thr = R.layout(layout)[2:]
    data = R.make_case(n, layout, min(b, n), seed=n + 7 * b)
    if n >= 255:                                         # two equal maxima in every eighth row, one sample without group 0
        data = R.with_equal_maxima(data, groups, thr, torch.arange(0, n, 8))
        lg = data['seg_logits'].clone()
        lg[data['batch_idx'] == 0, groups[0][0]] = -30.0
        data['seg_logits'] = lg
        assert bool(R.margin_ok(lg, groups, thr).all())
    det = detector(layout)
    batch = int(data['batch_idx'].max()) + 1
    d, out = run(det, data, batch)
    ref = R.group_sample(d, groups, thr)
    _check(d, out, ref, groups, 1, f'N = {n}, B = {b}')
    if n >= 255:
        assert ref['rule'][0] or len(groups[0]) > 1
    after_the_cluster_filter(det, d, out, ref, seed=n)


def test_refusals_by_name():
    data = {k: v.to(DEV) for k, v in R.make_case(40, 'small', 2, seed=3).items()}
    with pytest.raises(NotImplementedError, match='offset_weight'):
        _with(detector('small'), offset_weight='mean').sample(data, data['vote_offsets'])
    with pytest.raises(NotImplementedError, match='add_gt_fg_points'):
        _with(detector('small'), add_gt_fg_points=True).sample(data, data['vote_offsets'])
    with pytest.raises(NotImplementedError, match=r'num_classes \+ 1'):
        det = detector('small')
        det.sample(dict(data, seg_logits=data['seg_logits'][:, :3].contiguous()), data['vote_offsets'])
    with pytest.raises(NotImplementedError, match='two groups'):
        det = detector('small')
        det.cfg['group_names'] = [['b'], ['c', 'b']]
        det.sample(data, data['vote_offsets'])
    with pytest.raises(NotImplementedError, match='missing from class_names'):
        det = detector('small')
        det.cfg['group_names'] = [['b'], ['c', 'zebra']]
        det.sample(data, data['vote_offsets'])
    with pytest.raises(NotImplementedError, match='disable_pretrain_topks'):
        det = detector('small', training=True, runtime_info={}, disable_pretrain=True, disable_pretrain_topks=[5, 5, 5])
        det.sample(data, data['vote_offsets'])


def _with(det, **cfg):
    det.cfg.update(cfg)
    return det
