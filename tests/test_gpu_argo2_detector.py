"""SingleStageFSD built from configs/argo2/argo_onestage_12e.py (tests/golden/configs/argo2) with attach_heads(), on small
clouds: forward_train and simple_test over the grouped sampling kernels against the same modules called step by step through
the restatement's boolean indexing (tests/fsd_group_sample_ref.py), bit for bit; once with the per-class cluster assigner and
once with ``enable_class_batched``, both equal; and VoteSegmentor.forward_train of argo_segmentation_pretrain.py.  The stage
only copies rows and the library's kernels are deterministic; every grouped score the stage meets is clear of its threshold
(asserted)."""
import ast
import os

import pytest
import torch

import fsd_group_sample_ref as R
from conftest import GOLDEN
from test_gpu_fsd_detector import _same_losses, _total

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _model(name):
    return ast.literal_eval(open(os.path.join(GOLDEN, 'configs', 'argo2', name + '.model.py')).read())


def _scene():
    import bench_workloads as BW
    clouds = [BW.chain_cloud(2000, 5, half_extent=12.0)[:, :4].contiguous().to(DEV),
              BW.chain_cloud(1900, 6, half_extent=12.0)[:, :4].contiguous().to(DEV)]
    boxes, labels = [], []
    for s, cloud in enumerate(clouds):
        centre = cloud[[len(cloud) - 1, len(cloud) - 300, len(cloud) - 700], :3].cpu()
        b = torch.zeros(3, 7)
        b[:, :2], b[:, 2] = centre[:, :2], centre[:, 2] - 0.8
        b[:, 3:6], b[:, 6] = torch.tensor([1.6, 3.0, 1.6]), torch.tensor([0.3, -1.0, 2.0]) + s
        boxes.append(b.to(DEV))
        labels.append(torch.tensor([0, 1, 11], device=DEV))            # a vehicle, a pedestrian, a large vehicle: groups 0, 1, 3
    return clouds, boxes, labels


def _build():
    import sst_amd
    torch.manual_seed(0)
    det = sst_amd.build_detector(_model('argo_onestage_12e')).attach_heads().to(DEV)
    det.runtime_info = dict(enable_detection=True)
    return det


def _calibrate(det, clouds):
    """spread the untrained head's logits (standard deviation 2 per column) so that the groups select different points"""
    head = det.segmentor.segmentation_head
    with torch.no_grad():
        spread = 2.0 / det.segmentor([c.clone() for c in clouds])['seg_logits'].std(0)
        head.conv_seg.weight.mul_(spread[:, None])
        head.conv_seg.bias.mul_(spread)


def _groups(det, train):
    cfg = det.cfg
    groups = R.V.groups_by_names(cfg['group_names'], cfg['class_names'])
    return groups, R.thresholds32(cfg['score_thresh'], det.runtime_info.get('threshold_buffer', 0) if train else 0)


def _stage_by_indexing(det, seg_out, seg_feats, boxes, labels, train):
    det_ = (lambda t: t.detach()) if train else (lambda t: t)
    d = dict(seg_points=seg_out['seg_points'], seg_logits=det_(seg_out['seg_logits']), seg_vote_preds=det_(seg_out['seg_vote_preds']),
             seg_feats=seg_feats, batch_idx=seg_out['batch_idx'], vote_offsets=det_(seg_out['offsets']))
    d = det.pre_voxelize(d)
    groups, thr = _groups(det, train)
    assert bool(R.margin_ok(d['seg_logits'], groups, thr).all()), 'a grouped score of this scene is ambiguous against its threshold'
    smp = R.group_sample(d, groups, thr)
    inds, valid = det.cluster_assigner(smp['center_preds'], smp['batch_idx'], boxes, labels, origin_points=smp['seg_points'])
    upd = R.update_by_mask(smp, valid)
    comb = R.combine(upd)
    ext = det.extract_feat(comb['points'], comb['pts_feats'], torch.cat(inds, 0), None, comb['center_preds'])
    outs = det.bbox_head(ext['cluster_feats'], ext['cluster_xyz'], ext['cluster_inds'])
    return smp, comb, ext, outs


def _train_by_indexing(det, clouds, boxes, labels):
    metas = [{} for _ in clouds]
    seg_out = det.segmentor.forward_train(points=[c.clone() for c in clouds], img_metas=None, gt_bboxes_3d=boxes,
                                          gt_labels_3d=labels, as_subsegmentor=True)
    seg_feats = seg_out['seg_feats'].detach() if det.train_cfg.get('detach_segmentor', False) else seg_out['seg_feats']
    losses = dict(seg_out['losses'])
    smp, comb, ext, outs = _stage_by_indexing(det, seg_out, seg_feats, boxes, labels, True)
    losses['num_clusters'] = torch.ones((1,), device=DEV) * ext['cluster_xyz'].size(0)
    losses['num_fg_points'] = torch.ones((1,), device=DEV) * len(comb['points'])
    losses.update(det.bbox_head.loss(outs['cls_logits'], outs['reg_preds'], ext['cluster_xyz'], ext['cluster_inds'], boxes, labels,
                                     metas, iou_logits=outs.get('iou_logits', None)))
    return losses, smp, ext


def test_forward_train_per_class_and_class_batched():
    import sst_amd
    det = _build().train()
    clouds, boxes, labels = _scene()
    _calibrate(det, clouds)
    torch.manual_seed(1)
    losses = det.forward_train([c.clone() for c in clouds], [{} for _ in clouds], boxes, labels)
    assert {'loss_sem_seg', 'loss_vote', 'num_clusters', 'num_fg_points'} <= set(losses)
    assert {f'loss_cls.task{t}' for t in range(6)} <= set(losses)                 # one set of head losses per group
    _total(losses).backward()
    grads = {n: p.grad.clone() for n, p in det.named_parameters() if p.grad is not None}
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert float(next(g for n, g in grads.items() if n.startswith('backbone.')).abs().max()) > 0
    det.zero_grad(set_to_none=True)
    torch.manual_seed(1)
    want, smp, ext = _train_by_indexing(det, clouds, boxes, labels)
    assert len(smp['fg_mask_list']) == 6 and int(ext['cluster_inds'][:, 0].max()) <= 5      # column 0: the group = the task
    _same_losses(losses, want)
    assert sst_amd.enable_class_batched(det) == 1
    torch.manual_seed(1)
    batched = det.forward_train([c.clone() for c in clouds], [{} for _ in clouds], boxes, labels)
    _same_losses(batched, losses)
    _total(batched).backward()
    for n, p in det.named_parameters():
        if n in grads:
            assert torch.equal(p.grad, grads[n]), f'{n}: gradient differs with class_batched'


def test_simple_test_per_class_and_class_batched():
    import sst_amd
    det = _build().eval()
    clouds = _scene()[0][:1]
    _calibrate(det, clouds)
    with torch.no_grad():
        metas = [{}]
        got = det.simple_test([c.clone() for c in clouds], metas)
        seg_out = det.segmentor.simple_test([c.clone() for c in clouds], metas)
        smp, comb, ext, outs = _stage_by_indexing(det, seg_out, seg_out['seg_feats'], None, None, False)
        want = det.bbox_head.get_bboxes(outs['cls_logits'], outs['reg_preds'], ext['cluster_xyz'], ext['cluster_inds'], metas)
        sst_amd.enable_class_batched(det)
        batched = det.simple_test([c.clone() for c in clouds], metas)
    assert len(got) == len(want) == len(batched) == 1 and set(got[0]) == {'boxes_3d', 'scores_3d', 'labels_3d'}
    wb = getattr(want[0][0], 'tensor', want[0][0])
    for res in (got[0], batched[0]):
        gb = getattr(res['boxes_3d'], 'tensor', res['boxes_3d'])
        assert gb.size(0) > 0 and torch.equal(gb, wb.cpu())
        assert torch.equal(res['scores_3d'], want[0][1].cpu()) and torch.equal(res['labels_3d'], want[0][2].cpu())


def test_segmentation_pretrain_forward_train():
    import sst_amd
    torch.manual_seed(0)
    seg = sst_amd.build_detector(_model('argo_segmentation_pretrain')).to(DEV).train()
    clouds, boxes, labels = _scene()
    losses = seg.forward_train([c.clone() for c in clouds], [{} for _ in clouds], boxes, labels)
    assert {'loss_sem_seg', 'loss_vote', 'num_fg'} <= set(losses)
    assert all(bool(torch.isfinite(v).all()) for v in losses.values() if torch.is_tensor(v))
    (losses['loss_sem_seg'] + losses['loss_vote']).backward()
    assert any(p.grad is not None and float(p.grad.abs().max()) > 0 for p in seg.parameters())
