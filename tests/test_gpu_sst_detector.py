"""DynamicCenterPoint (sst_waymoD5_1x_3class_centerhead) and DynamicVoxelNet (sst_waymoD5_1x_3class_8heads_v2) with
attach_heads(): forward_train and simple_test on a grid of 4 x 4 windows against the same modules called one after the other.
The library's kernels are deterministic and the steps add no arithmetic of their own, so losses, gradients and boxes are compared
bit for bit."""
import ast
import os

import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SIDE = 48                                  # 4 windows of 12 voxels per side
HALF = SIDE * 0.32 / 2
PC = [-HALF, -HALF, -2, HALF, HALF, 4]
KEYS = {'DynamicCenterPoint': {'task0.loss_heatmap', 'task0.loss_bbox'}, 'DynamicVoxelNet': {'loss_cls', 'loss_bbox', 'loss_dir'}}
CONFIGS = {'DynamicCenterPoint': 'sst_waymoD5_1x_3class_centerhead', 'DynamicVoxelNet': 'sst_waymoD5_1x_3class_8heads_v2'}


def _model(kind):
    """the shipped model dictionary on a 48 x 48 grid with two blocks"""
    model = ast.literal_eval(open(os.path.join(GOLDEN, 'configs', 'sst_refactor', CONFIGS[kind] + '.model.py')).read())
    assert model['type'] == kind
    model['voxel_layer']['point_cloud_range'] = PC
    model['voxel_encoder']['point_cloud_range'] = PC
    # a deterministic voxel order (the shuffle draws from a device generator): two passes then see the same voxels in the same order
    model['middle_encoder'].update(sparse_shape=(SIDE, SIDE, 1), shuffle_voxels=False, window_major=True)
    bb = model['backbone']
    for key in ('d_model', 'nhead', 'dim_feedforward'):
        bb[key] = bb[key][:2]
    bb.update(num_blocks=2, output_shape=[SIDE, SIDE])
    if 'checkpoint_blocks' in bb:
        bb['checkpoint_blocks'] = []
    head = model['bbox_head']
    if kind == 'DynamicCenterPoint':
        head['bbox_coder'].update(pc_range=PC[:2], post_center_range=[-HALF, -HALF, -10.0, HALF, HALF, 10.0], max_num=200)
        model['train_cfg'].update(grid_size=[SIDE, SIDE, 1], point_cloud_range=PC, max_objs=40)
        model['test_cfg'].update(pc_range=PC[:2], pre_max_size=200, post_max_size=50, nms_pre=200)
    else:
        gen = head['anchor_generator']
        gen['ranges'] = [[-HALF, -HALF, r[2], HALF, HALF, r[5]] for r in gen['ranges']]
        model['test_cfg'].update(nms_pre=500, max_num=50)
    return model


def _build(kind, attach=True):
    import sst_amd
    torch.manual_seed(0)
    det = sst_amd.build_detector(_model(kind))
    if attach:
        det.attach_heads()
    det = det.to(DEV)
    if attach:
        with torch.no_grad():               # exercise the deformable path / let scores pass the thresholds
            for m in det.bbox_head.modules():
                if isinstance(m, sst_amd.DeformConv2dPack):
                    m.conv_offset.bias.copy_(torch.linspace(-1.3, 1.7, m.conv_offset.bias.numel(), device=DEV))
                    m.conv_offset.weight.normal_(0, 0.02)
            if kind == 'DynamicVoxelNet':
                det.bbox_head.conv_cls.weight.normal_(0, 0.05)
                det.bbox_head.conv_cls.bias.fill_(-2.0)
                det.bbox_head.conv_reg.weight.normal_(0, 0.02)
    return det


@pytest.fixture(autouse=True)
def _settled_torch_convolutions():
    """The attached convolutions, the neck and the heads' plain convolutions are torch's (MIOpen).  The first call of a shape may
    run another solver than the later ones (measured: the dilated 3 x 3 convolution differs by a few ulp between its first and its
    second call), so every comparison here is made after one warm-up pass, with the deterministic solvers asked for."""
    flag = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = flag


@pytest.fixture(scope='module')
def scene():
    import bench_workloads as BW
    clouds, centres = zip(*[BW.lidar_like_cloud(n, seed, DEV, half_extent=HALF - 0.3) for n, seed in ((3000, 3), (2600, 4))])
    boxes, labels = [], []
    for s, c in enumerate(centres):
        n = 5 - s
        b = torch.zeros(n, 9)
        b[:, :2], b[:, 2] = c[:n, :2], -1.8
        b[:, 3:6] = torch.tensor([[2.0, 4.5, 1.7], [0.8, 0.9, 1.7], [0.8, 1.8, 1.7], [2.1, 4.8, 1.6], [0.9, 0.9, 1.8]])[:n]
        b[:, 6] = torch.linspace(-1.2, 2.0, n)
        b[:, 7:] = torch.tensor([0.5, -0.25])
        boxes.append(b.to(DEV))
        labels.append(torch.tensor([0, 1, 2, 0, 1][:n], device=DEV))
    return list(clouds), boxes, labels


def _inputs(kind, scene):
    clouds, boxes, labels = scene
    cols = 5 if kind == 'DynamicCenterPoint' else 3            # the voxel encoders' in_channels
    box_cols = 9 if kind == 'DynamicCenterPoint' else 7
    return [c[:, :cols].contiguous() for c in clouds], [b[:, :box_cols].contiguous() for b in boxes], labels


def _flat(losses):
    return {k: (torch.stack(list(v)) if isinstance(v, (list, tuple)) else v) for k, v in losses.items()}


def _by_hand(det, kind, points, boxes, labels, metas):
    x = det.backbone(det.voxel_info([p.clone() for p in points]))
    feats = det.neck(x)
    outs = det.bbox_head(feats)
    if kind == 'DynamicCenterPoint':
        return det.bbox_head.loss(boxes, labels, outs)
    return det.bbox_head.loss(*outs, boxes, labels, metas, gt_bboxes_ignore=None)


def _step(det, points, boxes, labels, metas):
    det.zero_grad(set_to_none=True)
    torch.manual_seed(11)
    losses = _flat(det.forward_train([p.clone() for p in points], metas, boxes, labels))
    sum(v.sum() for v in losses.values()).backward()
    return losses, {n: p.grad.clone() for n, p in det.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('kind', list(CONFIGS))
def test_forward_train_is_the_modules_composed(kind, scene):
    det = _build(kind).train()
    points, boxes, labels = _inputs(kind, scene)
    metas = [dict() for _ in points]
    _step(det, points, boxes, labels, metas)             # warm-up: torch's convolution solvers settle
    losses, grads = _step(det, points, boxes, labels, metas)
    assert set(losses) == KEYS[kind]
    torch.manual_seed(11)
    want = _flat(_by_hand(det, kind, points, boxes, labels, metas))
    assert set(want) == set(losses)
    for k in want:
        assert bool(torch.isfinite(losses[k]).all()) and float(losses[k].detach().abs().sum()) > 0
        assert torch.equal(losses[k].detach().view(torch.int32), want[k].detach().view(torch.int32)), \
            f'{k}: {losses[k].tolist()} vs {want[k].tolist()}'
    import sst_amd
    for name, p in det.named_parameters():
        if name.startswith(('neck.', 'bbox_head.')):
            assert name in grads and bool(torch.isfinite(grads[name]).all()), name
    if kind == 'DynamicCenterPoint':
        packs = [m for m in det.bbox_head.modules() if isinstance(m, sst_amd.DeformConv2dPack)]
        assert len(packs) == 2
        for m in packs:
            for p in (m.weight, m.conv_offset.weight, m.conv_offset.bias):
                assert bool((p.grad != 0).any())
    # a second identical step: the same bits
    losses2, grads2 = _step(det, points, boxes, labels, metas)
    for k in losses:
        assert torch.equal(losses[k].detach().view(torch.int32), losses2[k].detach().view(torch.int32)), k
    assert set(grads) == set(grads2)
    for name in grads:
        assert torch.equal(grads[name].view(torch.int32), grads2[name].view(torch.int32)), name


@pytest.mark.parametrize('kind', list(CONFIGS))
def test_simple_test_is_get_bboxes_on_the_head_outputs(kind, scene):
    det = _build(kind).eval()
    points, _, _ = _inputs(kind, scene)
    metas = [dict() for _ in points]
    with torch.no_grad():
        det.simple_test([p.clone() for p in points], metas)            # warm-up
        torch.manual_seed(12)
        results = det.simple_test([p.clone() for p in points], metas)
        torch.manual_seed(12)
        outs = det.bbox_head(det.neck(det.backbone(det.voxel_info([p.clone() for p in points]))))
        want = det.bbox_head.get_bboxes(outs, metas) if kind == 'DynamicCenterPoint' else det.bbox_head.get_bboxes(*outs, metas)
    assert len(results) == len(points)
    cols = 9 if kind == 'DynamicCenterPoint' else 7
    for res, (boxes, scores, labels) in zip(results, want):
        assert set(res) == {'boxes_3d', 'scores_3d', 'labels_3d'}
        for v in res.values():
            assert not v.is_cuda
        n = res['scores_3d'].numel()
        assert n > 0 and tuple(res['boxes_3d'].shape) == (n, cols) and tuple(res['labels_3d'].shape) == (n,)
        assert torch.equal(res['boxes_3d'], boxes.cpu()) and torch.equal(res['scores_3d'], scores.cpu())
        assert torch.equal(res['labels_3d'], labels.cpu())


@pytest.mark.parametrize('kind', list(CONFIGS))
def test_without_attach_heads_nothing_changes(kind, scene):
    det = _build(kind, attach=False).eval()
    points, boxes, labels = _inputs(kind, scene)
    assert not any(k.startswith(('neck.', 'bbox_head.')) for k in det.state_dict())
    for call in (lambda: det.forward_train(points, [{}] * 2, boxes, labels), lambda: det.simple_test(points, [{}] * 2),
                 lambda: det.aug_test([points], [[{}] * 2])):
        with pytest.raises(NotImplementedError):
            call()
    with torch.no_grad():
        det.extract_feat([p.clone() for p in points])                  # warm-up
        torch.manual_seed(13)
        got = det.extract_feat([p.clone() for p in points])
        torch.manual_seed(13)
        want = det.backbone(det.voxel_info([p.clone() for p in points]))
    assert len(got) == len(want) == 1 and tuple(got[0].shape) == (2, 128, SIDE, SIDE)
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    attached = _build(kind).eval()
    with torch.no_grad():
        torch.manual_seed(13)
        out = attached.extract_feat([p.clone() for p in points])
    assert tuple(out[0].shape) == (2, attached.unbuilt['neck']['out_channels'][0], SIDE, SIDE)
