"""FSD and SingleStageFSD built from configs/fsd/fsd_waymoD1_1x.py with attach_heads(): forward_train and simple_test over the
sampling kernels against the same modules called step by step through the restatement's boolean indexing
(tests/fsd_sample_ref.py).  The forward pass of the stage only copies rows and the library's kernels are deterministic, so
losses and boxes are compared bit for bit; every logit the stage meets is 1e-6 clear of its threshold (asserted)."""
import ast
import os

import pytest
import torch

import fsd_sample_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SEG_KEYS = {'loss_sem_seg', 'loss_vote', 'recall_Car', 'recall_Ped', 'recall_Cyc'}
RPN_KEYS = {'num_clusters', 'num_fg_points'} | {f'{k}.task{t}' for k in ('loss_cls', 'loss_center', 'loss_size', 'loss_rot')
                                                for t in range(3)}      # SparseClusterHeadV2: one set of losses per task


def _build(kind='FSD', **train_cfg):
    import sst_amd
    model = ast.literal_eval(open(os.path.join(GOLDEN, 'configs', 'fsd', 'fsd_waymoD1_1x.model.py')).read())
    model['train_cfg'].update(train_cfg)
    if kind == 'SingleStageFSD':
        model['type'] = 'SingleStageFSD'
        model.pop('roi_head')
        model['bbox_head']['as_rpn'] = False
    torch.manual_seed(0)
    det = sst_amd.build_detector(model).attach_heads().to(DEV)
    det.runtime_info = dict(enable_detection=True)       # past the pre-training phase: thresholds, not top-k
    return det


def _scene():
    import bench_workloads as BW
    clouds = [BW.chain_cloud(2000, 5, half_extent=12.0).to(DEV), BW.chain_cloud(1900, 6, half_extent=12.0).to(DEV)]
    boxes, labels = [], []
    for s, cloud in enumerate(clouds):
        centre = cloud[[len(cloud) - 1, len(cloud) - 300, len(cloud) - 700], :3].cpu()
        b = torch.zeros(3, 7)
        b[:, :2], b[:, 2] = centre[:, :2], centre[:, 2] - 0.8
        b[:, 3:6], b[:, 6] = torch.tensor([1.6, 3.0, 1.6]), torch.tensor([0.3, -1.0, 2.0]) + s
        boxes.append(b.to(DEV))
        labels.append(torch.tensor([0, 1, 2], device=DEV))
    return clouds, boxes, labels


def _calibrate(det, clouds, empty_pair=False):
    """scale and bias the segmentation head's last layer so that every class selects between 5 % and 60 % of the points in the
    detector's current mode; with ``empty_pair`` class 2 then selects nothing in the last sample"""
    head = det.segmentor.segmentation_head
    head.__dict__.pop('forward', None)
    thr = torch.tensor(R.thresholds32(det.cfg['score_thresh']), device=DEV)
    with torch.no_grad():
        spread = 2.0 / det.segmentor([c.clone() for c in clouds])['seg_logits'].std(0)     # logits of standard deviation 2
        head.conv_seg.weight.mul_(spread[:, None])
        head.conv_seg.bias.mul_(spread)
        logits = det.segmentor([c.clone() for c in clouds])['seg_logits']
        want = torch.log(thr / (1 - thr))
        head.conv_seg.bias.add_(want - torch.quantile(logits, 0.7, dim=0))
        share = (det.segmentor([c.clone() for c in clouds])['seg_logits'].sigmoid() > thr[None]).float().mean(0)
    assert bool(((share > 0.05) & (share < 0.6)).all()), share
    if empty_pair:
        n0, plain = len(clouds[0]), type(head).forward

        def forward(voxel_feat):
            logits, votes = plain(head, voxel_feat)
            logits = logits.clone()
            logits[n0:, 2] = -50.0
            return logits, votes
        head.forward = forward


def _stage_by_indexing(det, seg_out, seg_feats, boxes, labels, train):
    """the stage between the segmentor and the heads through the restatement -> (dict_to_sample, final masks, points, extracted
    features, head outputs)"""
    det_ = (lambda t: t.detach()) if train else (lambda t: t)
    d = dict(seg_points=seg_out['seg_points'], seg_logits=det_(seg_out['seg_logits']), seg_vote_preds=det_(seg_out['seg_vote_preds']),
             seg_feats=seg_feats, batch_idx=seg_out['batch_idx'], vote_offsets=det_(seg_out['offsets']))
    d = det.pre_voxelize(d)
    thr = R.thresholds32(det.cfg['score_thresh'], det.runtime_info.get('threshold_buffer', 0) if train else 0)
    assert bool(R.margin_ok(d['seg_logits'], thr).all()), 'a logit of this scene is ambiguous against its threshold'
    smp = R.sample(d, thr)
    inds, valid = det.cluster_assigner(smp['center_preds'], smp['batch_idx'], boxes, labels, origin_points=smp['seg_points'])
    upd = R.update_by_mask(smp, valid)
    comb = R.combine(upd)
    ext = det.extract_feat(comb['points'], comb['pts_feats'], torch.cat(inds, 0), None, comb['center_preds'])
    outs = det.bbox_head(ext['cluster_feats'], ext['cluster_xyz'], ext['cluster_inds'])
    return d, smp, upd, comb, ext, outs


def _train_by_indexing(det, clouds, boxes, labels):
    metas = [{} for _ in clouds]
    seg_out = det.segmentor.forward_train(points=[c.clone() for c in clouds], img_metas=None, gt_bboxes_3d=boxes,
                                          gt_labels_3d=labels, as_subsegmentor=True)
    seg_feats = seg_out['seg_feats'].detach() if det.train_cfg.get('detach_segmentor', False) else seg_out['seg_feats']
    losses = dict(seg_out['losses'])
    d, smp, upd, comb, ext, outs = _stage_by_indexing(det, seg_out, seg_feats, boxes, labels, True)
    losses['num_clusters'] = torch.ones((1,), device=DEV) * ext['cluster_xyz'].size(0)
    losses['num_fg_points'] = torch.ones((1,), device=DEV) * len(comb['points'])
    losses.update(det.bbox_head.loss(outs['cls_logits'], outs['reg_preds'], ext['cluster_xyz'], ext['cluster_inds'], boxes, labels,
                                     metas, iou_logits=outs.get('iou_logits', None)))
    if hasattr(det, 'roi_head'):
        proposals = det.bbox_head.get_bboxes(outs['cls_logits'], outs['reg_preds'], ext['cluster_xyz'], ext['cluster_inds'], metas)
        pts, feats, bidx = R.roi_multi(d['seg_points'], ext['cluster_pts_feats'], d['seg_feats'], upd['fg_mask_list'], d['batch_idx'])
        losses.update(det.roi_head.forward_train(pts, feats, bidx, metas, proposals, boxes, labels))
    return losses, smp


def _total(losses):
    return sum(v.sum() if torch.is_tensor(v) else sum(x.sum() for x in v)
               for k, v in losses.items() if (torch.is_tensor(v) and v.requires_grad) or isinstance(v, (list, tuple)))


def _same_losses(got, want):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in want:
        a, b = got[k], want[k]
        a, b = (torch.stack(list(a)), torch.stack(list(b))) if isinstance(b, (list, tuple)) else (a, b)
        assert bool(torch.isfinite(a).all()), f'{k} is not finite'
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), f'{k}: {a.tolist()} vs {b.tolist()}'


@pytest.mark.parametrize('kind,empty_pair', [('FSD', False), ('FSD', True), ('SingleStageFSD', False)])
def test_forward_train(kind, empty_pair):
    det = _build(kind).train()
    clouds, boxes, labels = _scene()
    _calibrate(det, clouds, empty_pair)
    torch.manual_seed(1)
    losses = det.forward_train([c.clone() for c in clouds], [{} for _ in clouds], boxes, labels)
    assert SEG_KEYS | RPN_KEYS <= set(losses)
    if kind == 'FSD':
        assert any(k.startswith('loss_rcnn_') for k in losses) and {'loss_rcnn_cls', 'loss_rcnn_bbox'} <= set(losses)
    _total(losses).backward()
    got_grads = {n: p.grad.clone() for n, p in det.named_parameters() if p.grad is not None}
    det.zero_grad(set_to_none=True)
    torch.manual_seed(1)
    want, smp = _train_by_indexing(det, clouds, boxes, labels)
    if empty_pair:
        assert smp['rule'] == [False, False, True], 'class 2 selects nothing in the last sample: the rule gives it a point per sample'
    _same_losses(losses, want)
    _total(want).backward()
    for name, p in det.named_parameters():
        if p.grad is not None:
            assert name in got_grads and bool(torch.isfinite(got_grads[name]).all()), name
    assert float(got_grads['backbone.block_list.0.pre_mlp.0.0.weight' if 'backbone.block_list.0.pre_mlp.0.0.weight' in got_grads
                           else next(n for n in got_grads if n.startswith('backbone.'))].abs().max()) > 0


def test_detach_segmentor():
    """with train_cfg.detach_segmentor the segmentor's gradients are those of its own losses alone"""
    det = _build('FSD', detach_segmentor=True).train()
    clouds, boxes, labels = _scene()
    _calibrate(det, clouds)
    torch.manual_seed(1)
    losses = det.forward_train([c.clone() for c in clouds], [{} for _ in clouds], boxes, labels)
    params = [p for p in det.segmentor.parameters() if p.requires_grad]
    own = torch.autograd.grad(losses['loss_sem_seg'] + losses['loss_vote'], params, retain_graph=True, allow_unused=True)
    every = torch.autograd.grad(_total(losses), params, allow_unused=True)
    for (name, _), a, b in zip(det.segmentor.named_parameters(), own, every):
        assert (a is None) == (b is None), name
        if a is not None:
            assert torch.equal(a, b), f'{name}: the detached stage sent a gradient into the segmentor'


def _same_boxes(got, want):
    assert len(got) == len(want) == 1
    for g, w in zip(got, want):
        gb, wb = (getattr(x[0], 'tensor', x[0]) for x in (g, w))
        assert torch.equal(gb, wb) and torch.equal(g[1], w[1]) and torch.equal(g[2], w[2])
        assert gb.size(0) > 0


def test_simple_test():
    det = _build('FSD').eval()
    clouds, boxes, labels = _scene()
    clouds = clouds[:1]
    _calibrate(det, clouds)
    with torch.no_grad():
        metas = [{}]
        got = det.simple_test([c.clone() for c in clouds], metas)
        seg_out = det.segmentor.simple_test([c.clone() for c in clouds], metas)
        d, smp, upd, comb, ext, outs = _stage_by_indexing(det, seg_out, seg_out['seg_feats'], None, None, False)
        proposals = det.bbox_head.get_bboxes(outs['cls_logits'], outs['reg_preds'], ext['cluster_xyz'], ext['cluster_inds'], metas)
        pts, feats, bidx = R.roi_multi(d['seg_points'], ext['cluster_pts_feats'], d['seg_feats'], upd['fg_mask_list'], d['batch_idx'])
        want = det.roi_head.simple_test(pts, feats, bidx, metas, proposals, None, None)
        _same_boxes(got, want)
        det.test_cfg['skip_rcnn'] = True
        skipped = det.simple_test([c.clone() for c in clouds], metas)
    assert len(skipped) == 1 and set(skipped[0]) == {'boxes_3d', 'scores_3d', 'labels_3d'}
    pb = getattr(proposals[0][0], 'tensor', proposals[0][0])
    sb = getattr(skipped[0]['boxes_3d'], 'tensor', skipped[0]['boxes_3d'])
    assert torch.equal(sb, pb.cpu()) and torch.equal(skipped[0]['scores_3d'], proposals[0][1].cpu())
    assert torch.equal(skipped[0]['labels_3d'], proposals[0][2].cpu())


def _g(array):
    import numpy as np
    return torch.from_numpy(np.ascontiguousarray(array))      # the file stores its matrices column-major


def test_pre_voxelize_against_the_golden():
    """new_coors and the inverse equal torch.unique(dim=0); the averaged features within 1e-5 of the float64 means"""
    from conftest import load_golden
    gold = load_golden('fsd_sample.npz')
    det = _build('SingleStageFSD')
    det.cfg = dict(det.cfg, pre_voxelization_size=(0.5, 0.5, 0.5))
    det.cluster_assigner.point_cloud_range = [float(x) for x in gold['pv_pc_range']]
    keys = ('seg_points', 'seg_logits', 'seg_vote_preds', 'seg_feats', 'batch_idx', 'vote_offsets')
    out = det.pre_voxelize({k: _g(gold[f'pv_in_{k}']).to(DEV) for k in keys})
    assert set(out) == set(keys)
    assert torch.equal(out['batch_idx'].cpu(), _g(gold['pv_new_coors'][:, 0]))
    for k in keys:
        if k != 'batch_idx':
            ref = gold[f'pv_out_f64_{k}'] if f'pv_out_f64_{k}' in gold else gold[f'pv_out_{k}']
            err = float((out[k].cpu().double() - _g(ref).double()).abs().max())
            assert out[k].shape == ref.shape and err < 1e-5, (k, err)
    from sst_amd.sst_ops import unique_with_plan
    pts, bidx = _g(gold['pv_in_seg_points']).to(DEV), _g(gold['pv_in_batch_idx']).to(DEV)
    lo = torch.tensor(gold['pv_pc_range'][:3], dtype=torch.float32, device=DEV)
    coors = torch.div(pts[:, :3] - lo[None], torch.tensor([0.5, 0.5, 0.5], device=DEV)[None], rounding_mode='floor').long()
    new_coors, inv = unique_with_plan(torch.cat([bidx[:, None], coors[:, [2, 1, 0]]], 1))
    assert torch.equal(new_coors.cpu(), _g(gold['pv_new_coors'])) and torch.equal(inv.cpu(), _g(gold['pv_unq_inv']))
