"""The FSD cluster heads without a GPU: the restatement of tests/cluster_head_ref.py against the reference's own methods
(tests/golden/cluster_head_train.npz), the construction of SparseClusterHeadV2 / FSDV2Head from every shipped fsd / fsdv2 config,
the refused keys, and the loud failures of the Python entry points on CPU tensors."""
import ast
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

import cluster_head_ref as R

# every fsd / fsdv2 fixture that is a detector with a box head (fsd_sst_encoder_pretrain is the segmentor alone)
FSD_CONFIGS = sorted(os.path.relpath(p, os.path.join(GOLDEN, 'configs'))[:-len('.model.py')]
                     for d in ('fsd', 'fsdv2') for p in glob.glob(os.path.join(GOLDEN, 'configs', d, '*.model.py'))
                     if 'bbox_head' in ast.literal_eval(open(p).read()))
# case -> (tasks, class names, box columns, label key, width tag, centroid_assign, rows without sample 2)
CASES = {}
for _tag in R.WIDTHS:
    CASES[f'waymo_{_tag}'] = (R.WAYMO_TASKS, R.WAYMO_NAMES, 7, 'labels_waymo', _tag, False, False)
    CASES[f'multi_{_tag}'] = (R.MULTI_TASKS, R.MULTI_NAMES, 10, 'labels_multi', _tag, False, False)
CASES['multi_centroid'] = (R.MULTI_TASKS, R.MULTI_NAMES, 10, 'labels_multi', 'p03', True, False)
CASES['waymo_norows'] = (R.WAYMO_TASKS, R.WAYMO_NAMES, 7, 'labels_waymo', 'none', False, True)


@pytest.fixture(scope='module')
def gold():
    return load_golden('cluster_head_train.npz')


def scene(gold, case):
    tasks, names, cols, lkey, tag, centroid, norows = CASES[case]
    rows = gold['cluster_inds'][:, 1] != 2 if norows else np.ones(len(gold['xyz']), bool)
    xyz, aux = gold['xyz'][rows], gold['aux_xyz'][rows]
    return dict(tasks=tasks, names=names, code=8 if cols == 7 else 10, width=R.WIDTHS[tag], rows=rows, xyz=xyz,
                xyz_assign=aux if centroid else xyz, cluster_inds=gold['cluster_inds'][rows],
                boxes=[gold[f'boxes{s}'][:, :cols] for s in range(3)], labels=[gold[f'{lkey}{s}'] for s in range(3)],
                code_weight=R.CODE_WEIGHT10 if cols == 10 else None)


def restated_targets(sc, dtype=torch.float32):
    return R.targets(sc['xyz_assign'], sc['xyz'], sc['cluster_inds'][:, 1], sc['boxes'], sc['labels'], sc['tasks'], sc['names'],
                     sc['code'], sc['width'], dtype)


@pytest.mark.parametrize('case', list(CASES))
def test_restated_targets_equal_the_reference(gold, case):
    sc = scene(gold, case)
    for t, (lab, assigned, tg, wt) in enumerate(restated_targets(sc)):
        pre = f'{case}_t{t}_'
        assert np.array_equal(lab.numpy(), gold[pre + 'labels'])
        assert np.array_equal(assigned.numpy(), gold[pre + 'assigned'])
        g_tg = gold[pre + 'bbox_targets']
        plain = [0, 1, 2] + ([8, 9] if sc['code'] == 10 else [])
        assert np.array_equal(tg.numpy()[:, plain], g_tg[:, plain])
        assert np.array_equal(wt.numpy(), gold[pre + 'bbox_weights'])
        assert R.ulp_distance(tg.numpy()[:, 3:8], g_tg[:, 3:8]).max() <= 1       # log / sin / cos on other array shapes


def test_the_scene_holds_the_cases_the_targets_must_get_right(gold):
    inds = gold['cluster_inds']
    assert (np.diff(inds[:, 0]) >= 0).all() and (np.diff(inds[:, 1]) != 0).sum() > 100      # class-major: samples interleave
    assert len(gold['boxes1']) == 0 and (inds[:, 1] == 1).sum() > 50                         # the middle sample has no box
    assert (gold['labels_waymo0'] == -1).sum() == 1 and (gold['labels_multi2'] == -1).sum() == 1
    assert 550 <= len(inds) <= 650
    # a task without a positive row
    assert (gold['waymo_none_t2_assigned'] < 0).all() and float(gold['waymo_none_t2_f64_loss_center']) == 0.0
    # the overlap of box 0 (car: index 1 of task 0) and box 1 (bus: index 0) goes to box 1, against the index order
    import seg_loss_ref as S
    hit = S.inside(gold['boxes0'][:2, :7], gold['xyz']) & (inds[:, 1] == 0)[None]
    both = hit[0] & hit[1]
    assert both.sum() >= 3 and (gold['multi_none_t0_assigned'][both] == 1).all() and (gold['multi_none_t0_labels'][both] == 0).all()
    assert (gold['waymo_none_t0_assigned'][both] == 0).all()          # one class per task: the index order decides
    # the widths move the assignment; the thin box keeps its extents at the negative width
    for fam in ('waymo', 'multi'):
        a = [gold[f'{fam}_{tag}_t0_assigned'] for tag in R.WIDTHS]
        assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[0], a[2])
    assert (gold['waymo_m02_t0_assigned'] == 2).sum() > 0
    # copy-paste flags 0 and 1 on positive rows; centroid_assign moves the assignment but not the base of the regression
    w = gold['multi_none_t0_bbox_weights']
    assert ((w[:, 8] == 0) & (w[:, 0] == 1)).any() and ((w[:, 8] == 1) & (w[:, 9] == 1)).any()
    assert not np.array_equal(gold['multi_centroid_t0_assigned'], gold['multi_p03_t0_assigned'])
    # no tested point within 1e-3 m of a face of any (enlarged) box
    every = np.concatenate([gold['boxes0'][:, :7], gold['boxes2'][:, :7]])
    assert not R.near_a_face(every, gold['xyz']).any() and not R.near_a_face(every, gold['aux_xyz']).any()
    assert (np.abs(gold['waymo_logits0'].astype(np.float32)) == 60).sum() >= 4


@pytest.mark.parametrize('case', R.LOSS_CASES)
def test_restated_losses_equal_the_reference(gold, case):
    sc = scene(gold, case)
    fam = case.split('_')[0]
    for t, (lab, assigned, tg, wt) in enumerate(restated_targets(sc, torch.float64)):
        pre = f'{case}_t{t}_'
        got = R.losses_and_grads(gold[f'{fam}_logits{t}'].astype(np.float32)[sc['rows']],
                                 gold[f'{fam}_reg{t}'].astype(np.float32)[sc['rows']], lab, tg, wt, code_weight=sc['code_weight'])
        assert got['status'] == 0 and got['num_pos'] == int((gold[pre + 'assigned'] >= 0).sum())
        for name in R.LOSS_NAMES[:sc['code'] // 2]:
            ref = float(gold[pre + 'f64_' + name])
            assert abs(got[name] - ref) <= 1e-12 * max(abs(ref), 1e-30), name
            assert 0 <= float(gold[f'noise_{pre}{name}']) < 1e-5
        for k in ('d_logits', 'd_reg'):
            ref = gold[pre + 'f64_' + k]
            assert np.array_equal(got[k].numpy() != 0, ref != 0)
            assert np.abs(got[k].numpy() - ref).max() <= 1e-12 * np.abs(ref).max()
            assert 0 <= float(gold[f'noise_{pre}{k}']) < 1e-5


def _model_cfg(name):
    return ast.literal_eval(open(os.path.join(GOLDEN, 'configs', name + '.model.py')).read())


def _head_cfg(model):
    return dict(model['bbox_head'], train_cfg=model.get('train_cfg'), test_cfg=model.get('test_cfg'))


@pytest.mark.parametrize('name', FSD_CONFIGS)
def test_heads_build_from_every_fsd_and_fsdv2_config(name):
    import sst_amd
    assert len(FSD_CONFIGS) == 10
    model = _model_cfg(name)
    cfg = model['bbox_head']
    head = sst_amd.build_head(_head_cfg(model))
    assert type(head).__name__ == cfg['type'] and cfg['type'] in ('SparseClusterHeadV2', 'FSDV2Head')
    assert isinstance(head.bbox_coder, sst_amd.BasePointBBoxCoder)
    code = cfg['bbox_coder'].get('code_size', 8)
    assert head.box_code_size == code and len(head.task_heads) == len(cfg['tasks'])
    sd = head.state_dict()
    dims = [cfg['in_channel']] + list(cfg['shared_mlp_dims'])
    for i in range(len(dims) - 1):
        assert tuple(sd[f'shared_mlp.{i}.0.weight'].shape) == (dims[i + 1], dims[i])
        assert f'shared_mlp.{i}.0.bias' not in sd and tuple(sd[f'shared_mlp.{i}.1.weight'].shape) == (dims[i + 1],)
    attrs = dict(cfg['common_attrs'])
    for t, task in enumerate(cfg['tasks']):
        attrs['score'] = (len(task['class_names']), cfg['num_cls_layer'], cfg['cls_hidden_dim'])
        assert set(head.task_heads[t].attrs) == set(attrs)
        for attr, (out_dim, layers, hidden) in attrs.items():
            width = dims[-1]
            for i in range(layers):
                assert tuple(sd[f'task_heads.{t}.{attr}.{i}.0.weight'].shape) == (hidden, width)
                width = hidden
            assert tuple(sd[f'task_heads.{t}.{attr}.{layers}.weight'].shape) == (out_dim, width)
            assert tuple(sd[f'task_heads.{t}.{attr}.{layers}.bias'].shape) == (out_dim,)
    # nothing but the shared MLP and the task heads: the keys a reference checkpoint's bbox_head.* entries have
    assert all(k.startswith(('shared_mlp.', 'task_heads.')) for k in sd)
    assert head.conv_cls is None and head.conv_reg is None
    # the detector keeps parking the head's config, exactly as before
    det = sst_amd.build_detector(model)
    assert det.unbuilt['bbox_head'] == cfg
    assert not any(k.startswith('bbox_head.') for k in det.state_dict())


def test_fsd_waymo_head_has_the_expected_shapes():
    import sst_amd
    head = sst_amd.build_head(_head_cfg(_model_cfg('fsd/fsd_waymoD1_1x')))
    sd = head.state_dict()
    assert tuple(sd['shared_mlp.0.0.weight'].shape) == (1024, 768) and tuple(sd['shared_mlp.1.0.weight'].shape) == (1024, 1024)
    assert len(head.task_heads) == 3
    for t in range(3):
        for attr, out in (('center', 3), ('dim', 3), ('rot', 2), ('score', 1)):
            assert tuple(sd[f'task_heads.{t}.{attr}.0.0.weight'].shape) == (128, 1024)
            assert tuple(sd[f'task_heads.{t}.{attr}.1.0.weight'].shape) == (128, 128)
            assert tuple(sd[f'task_heads.{t}.{attr}.2.weight'].shape) == (out, 128)
    out = head(torch.randn(7, 768))
    assert [tuple(t.shape) for t in out['cls_logits']] == [(7, 1)] * 3 and [tuple(t.shape) for t in out['reg_preds']] == [(7, 8)] * 3
    nusc = sst_amd.build_head(_head_cfg(_model_cfg('fsdv2/fsdv2_nusc_1x')))
    out = nusc(torch.randn(7, 128))
    assert [tuple(t.shape) for t in out['cls_logits']] == [(7, 5)] * 2 and [tuple(t.shape) for t in out['reg_preds']] == [(7, 10)] * 2
    assert isinstance(nusc.shared_mlp[0][1], sst_amd.NaiveSyncBatchNorm1d)
    assert nusc.loss_weights == [4.0, 0.5, 0.5, 0.2, 0.2] and head.loss_weights == [2.0, 0.5, 0.5, 0.2, 0.0]
    # fsdv2_argo_2x regresses with SmoothL1Loss (beta 0.1): built, not refused
    argo = sst_amd.build_head(_head_cfg(_model_cfg('fsdv2/fsdv2_argo_2x')))
    assert argo.smooth_l1_beta == [0.0, 0.1, 0.1, 0.1, 0.0] and head.smooth_l1_beta == [0.0] * 5


def _small_cfg(**over):
    cfg = dict(type='SparseClusterHeadV2', num_classes=3, bbox_coder=dict(type='BasePointBBoxCoder'),
               loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
               loss_center=dict(type='L1Loss', loss_weight=0.5), loss_size=dict(type='L1Loss', loss_weight=0.5),
               loss_rot=dict(type='L1Loss', loss_weight=0.2), in_channel=16, shared_mlp_dims=[16], tasks=R.WAYMO_TASKS,
               class_names=R.WAYMO_NAMES, common_attrs=dict(center=(3, 1, 8), dim=(3, 1, 8), rot=(2, 1, 8)), num_cls_layer=1,
               cls_hidden_dim=8, separate_head=dict(type='FSDSeparateHead', norm_cfg=dict(type='LN'), act='relu'),
               train_cfg=dict(), test_cfg=dict())
    cfg.update(over)
    return cfg


@pytest.mark.parametrize('key, over', [
    ('loss_iou', dict(loss_iou=dict(type='CrossEntropyLoss', use_sigmoid=True))),
    ('iou_mlp', dict(iou_mlp=[16])),
    ('corner_loss_cfg', dict(corner_loss_cfg=dict(delta=1.0, loss_weight=1.0))),
    ('enlarge_width', dict(enlarge_width=dict(strategy='scale', scale=1.2))),
    ('loss_cls', dict(loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True))),
    ('loss_cls', dict(loss_cls=dict(type='FocalLoss', use_sigmoid=False))),
    ('loss_center', dict(loss_center=dict(type='MSELoss'))),
    ('loss_size', dict(loss_size=dict(type='L1Loss', reduction='sum'))),
    ('loss_rot', dict(loss_rot=dict(type='SmoothL1Loss', beta=0.0))),
    ('loss_vel', dict(loss_vel=dict(type='MSELoss'))),
])
@pytest.mark.parametrize('kind', ['SparseClusterHeadV2', 'FSDV2Head'])
def test_unbuilt_constructor_keys_are_refused_by_name(kind, key, over):
    import sst_amd
    with pytest.raises(NotImplementedError, match=key):
        sst_amd.build_head(_small_cfg(type=kind, **over))


@pytest.mark.parametrize('key, value', [('assign_by_dist', True), ('max_assign_dist', [1.0, 1.0, 1.0])])
def test_unbuilt_train_cfg_keys_are_refused_when_used(key, value):
    import sst_amd
    head = sst_amd.build_head(_small_cfg(train_cfg={key: value}))       # construction is fine: the key is a train_cfg key
    xyz = torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match=key):
        head.get_targets(1, xyz, torch.zeros(4, dtype=torch.long), [torch.zeros(0, 7)], [torch.zeros(0, dtype=torch.long)])
    with pytest.raises(NotImplementedError, match=key):
        head.loss([torch.zeros(4, 1)] * 3, [torch.zeros(4, 8)] * 3, xyz, torch.zeros(4, 3, dtype=torch.long), [torch.zeros(0, 7)],
                  [torch.zeros(0, dtype=torch.long)])


def test_detach_yaw_is_refused():
    import sst_amd
    coder = sst_amd.BasePointBBoxCoder(code_size=8)
    with pytest.raises(NotImplementedError, match='detach_yaw'):
        coder.decode(torch.zeros(2, 8), torch.zeros(2, 3), detach_yaw=True)
    assert sst_amd.BBOX_CODERS.build(dict(type='BasePointBBoxCoder', code_size=10)).code_size == 10


def test_ops_raise_on_cpu_tensors(gold):
    import sst_amd
    sc = scene(gold, 'waymo_none')
    xyz, inds = torch.from_numpy(sc['xyz']), torch.from_numpy(sc['cluster_inds'])
    boxes, labels = [torch.from_numpy(b) for b in sc['boxes']], [torch.from_numpy(l) for l in sc['labels']]
    with pytest.raises(RuntimeError):
        sst_amd.cluster_targets(xyz, inds, boxes, labels, sc['tasks'], sc['names'], 8)
    n = len(xyz)
    logits, reg = [torch.zeros(n, 1)] * 3, [torch.zeros(n, 8)] * 3
    with pytest.raises(RuntimeError):
        sst_amd.cluster_loss(logits, reg, [torch.zeros(n, dtype=torch.long)] * 3, reg, reg)
    with pytest.raises(RuntimeError):
        sst_amd.cluster_decode(reg[0], xyz, logits[0])
    with pytest.raises(RuntimeError):
        sst_amd.cluster_encode(boxes[0], xyz[:len(boxes[0])])
    head = sst_amd.build_head(_small_cfg())
    with pytest.raises(RuntimeError):
        head.loss(logits, reg, xyz, inds, boxes, labels)
    with pytest.raises(RuntimeError):
        head.get_bboxes(logits, reg, xyz, inds, [dict()] * 3)
