"""The Argoverse 2 FSD family without a GPU: both shipped configs (tests/golden/configs/argo2, resolved by
tests/golden/make_argo2_fixtures.py) construct through the registry, ``attach_heads()`` of argo_onestage_12e builds the 6-task
SparseClusterHeadV2, the pipelines and the training settings are taken as shipped, the fixtures equal the config text where
the reference exists, and the cluster assigner reads the family's list-valued tables per class."""
import ast
import copy
import glob
import os

import pytest

from test_configs_build import FIXTURES, REF, load_config

NAMES = ('argo_onestage_12e', 'argo_segmentation_pretrain')
TRAIN_KEYS = ('fp16', 'lr_config', 'momentum_config', 'optimizer', 'optimizer_config', 'runner')


def fixture(name, kind='model'):
    return ast.literal_eval(open(os.path.join(FIXTURES, 'argo2', f'{name}.{kind}.py')).read())


def test_the_shipped_configs_have_fixtures():
    have = sorted(os.path.basename(p) for p in glob.glob(os.path.join(FIXTURES, 'argo2', '*.py')))
    assert have == sorted(f'{n}.{k}.py' for n in NAMES for k in ('model', 'pipeline', 'train'))


@pytest.mark.parametrize('name', NAMES)
def test_fixtures_equal_the_config_text(name):
    path = os.path.join(REF, 'configs', 'argo2', name + '.py')
    if not os.path.exists(path):
        pytest.skip('the reference tree is not on this machine')
    cfg = load_config(path)
    assert cfg['model'] == fixture(name) and repr(cfg['model']) == repr(fixture(name))
    assert {k: cfg[k] for k in ('train_pipeline', 'test_pipeline')} == fixture(name, 'pipeline')
    assert {k: cfg.get(k) for k in TRAIN_KEYS} == fixture(name, 'train')


def test_the_family_is_the_long_range_case():
    model = fixture('argo_onestage_12e')
    seg = model['segmentor']
    assert seg['voxel_layer']['point_cloud_range'] == [-204.8, -204.8, -3.2, 204.8, 204.8, 3.2]
    assert seg['backbone']['sparse_shape'] == [32, 2048, 2048]
    assert len(model['train_cfg']['class_names']) == 26 and [len(g) for g in model['train_cfg']['group_names']] == [1, 4, 6, 9, 5, 1]
    assert model['train_cfg']['group_sample'] is True and model['test_cfg']['group_sample'] is True
    assert len(model['bbox_head']['tasks']) == 6


def test_onestage_constructs_and_attaches_the_six_task_head():
    import sst_amd
    det = sst_amd.build_detector(copy.deepcopy(fixture('argo_onestage_12e')))
    assert type(det).__name__ == 'SingleStageFSD' and type(det.segmentor).__name__ == 'VoteSegmentor'
    assert det.num_classes == 26 and det.cluster_assigner.num_classes == 26 and det.cluster_assigner.class_batched is False
    assert det.segmentor.segmentation_head.conv_seg.out_features == 27          # softmax head: 26 classes + background
    assert det.segmentor.segmentation_head.loss_mode == 'softmax_ce' and not det.segmentor.segmentation_head.loss_unbuilt
    keys = list(det.state_dict())
    det.attach_heads()
    assert type(det.bbox_head).__name__ == 'SparseClusterHeadV2' and len(det.bbox_head.tasks) == 6
    assert len(det.state_dict()) > len(keys) and list(det.state_dict())[:len(keys)] == keys
    assert sst_amd.enable_class_batched(det) == 1 and det.cluster_assigner.class_batched


def test_segmentation_pretrain_constructs():
    import sst_amd
    seg = sst_amd.build_detector(copy.deepcopy(fixture('argo_segmentation_pretrain')))
    assert type(seg).__name__ == 'VoteSegmentor' and seg.num_classes == 26
    head = seg.segmentation_head
    assert head.loss_mode == 'softmax_ce' and not head.loss_unbuilt and head.num_classes == 27 <= 32
    assert len(head.loss_args['class_weight']) == 27


def test_cluster_assigner_reads_the_list_tables_per_class():
    import sst_amd
    cfg = fixture('argo_onestage_12e')['cluster_assigner']
    a = sst_amd.ClusterAssigner(**cfg)
    names = a.class_names
    assert [a._per_class(a.cluster_voxel_size, c) for c in names[:6]] == \
        [(0.3, 0.3, 6.4), (0.05, 0.05, 6.4), (0.08, 0.08, 6.4), (0.5, 0.5, 6.4), (0.1, 0.1, 6.4), (0.08, 0.08, 6.4)]
    assert [a._per_class(a.connected_dist, c) for c in names[:6]] == [0.6, 0.1, 0.15, 1.0, 0.2, 0.15]
    assert a.min_points == 2 and a.point_cloud_range[:3] == [-204.8, -204.8, -3.2]


def _detector(**train_cfg):
    import sst_amd
    model = copy.deepcopy(fixture('argo_onestage_12e'))
    model['train_cfg'].update(train_cfg)
    det = sst_amd.build_detector(model).train()
    det.runtime_info = dict(enable_detection=True)
    return det


def _rows(n=8, width=27):
    import torch
    return dict(seg_points=torch.zeros(n, 4), seg_logits=torch.zeros(n, width), seg_vote_preds=torch.zeros(n, 3 * width),
                seg_feats=torch.zeros(n, 8), batch_idx=torch.zeros(n, dtype=torch.long), vote_offsets=torch.zeros(n, 3 * width))


@pytest.mark.parametrize('change,exc,match', [
    (dict(offset_weight='mean'), NotImplementedError, "offset_weight 'mean'"),
    (dict(add_gt_fg_points=True), NotImplementedError, 'add_gt_fg_points with group_sample'),
    (dict(group_names=[['Regular_vehicle'], ['Pedestrian', 'Regular_vehicle']], score_thresh=[0.4, 0.25]), NotImplementedError,
     'listed in two groups'),
    (dict(group_names=[['Regular_vehicle'], ['Zebra']], score_thresh=[0.4, 0.25]), NotImplementedError, "'Zebra' is missing"),
    (dict(group_names=[['Regular_vehicle'], []], score_thresh=[0.4, 0.25]), NotImplementedError, 'lists no class'),
    (dict(score_thresh=[0.4, 0.25]), RuntimeError, '6 groups for 2 score thresholds'),
    (dict(disable_pretrain=True, disable_pretrain_topks=[100, 100, 100]), NotImplementedError, 'disable_pretrain_topks has 3 entries'),
])
def test_group_sample_refuses_by_name_before_it_touches_the_device(change, exc, match):
    """host tensors: a call that got past its refusals would fail on them with another message"""
    det = _detector(**change)
    if 'disable_pretrain' in change:
        det.runtime_info = {}
    data = _rows()
    with pytest.raises(exc, match=match):
        det.sample(data, data['vote_offsets'], batch_size=1)


def test_group_sample_refuses_logits_of_the_wrong_width():
    det = _detector()
    for width in (26, 28):
        data = _rows(width=width)
        with pytest.raises(NotImplementedError, match=r'num_classes \+ 1 = 27'):
            det.sample(data, data['vote_offsets'], batch_size=1)
    det.cfg['group_sample'] = False                      # the per-class path keeps its own refusal of a background column
    with pytest.raises(NotImplementedError, match='background column'):
        det.sample(_rows(), _rows()['vote_offsets'], batch_size=1)


@pytest.mark.parametrize('name', NAMES)
def test_pipelines_and_training_settings_are_taken_as_shipped(name):
    import torch
    from sst_amd import optim
    from sst_amd.augment import TrainAugment
    pipes = fixture(name, 'pipeline')
    train = TrainAugment.from_pipeline(pipes['train_pipeline'])
    test = TrainAugment.from_pipeline(pipes['test_pipeline'])
    assert train is not None and test is not None
    update, schedules = optim.build_training_update(torch.nn.Linear(4, 4), fixture(name, 'train'), max_iters=100)
    assert update is not None and schedules
