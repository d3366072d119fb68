"""FSDV2 (configs/fsdv2/fsdv2_waymo_1x.py: per-class sigmoid path, as_rpn, RoI head, pre_2nd_voxelization) and SingleStageFSDV2
(configs/fsdv2/fsdv2_nusc_1x.py: batched_group_sample, centroid_assign) built with build_detector + attach_fsdv2_heads:
forward_train and simple_test over the sampling kernels against the same modules called step by step through the restatements'
boolean indexing (tests/fsdv2_sample_ref.py, tests/fsd_sample_ref.py).  The stage only copies rows and does the centre arithmetic
of tests/test_gpu_fg_group_sample.py, and the library's kernels are deterministic, so losses and boxes are compared bit for bit;
every logit the stage meets is clear of its threshold by the restatement's margin (asserted)."""
import ast
import os

import numpy as np
import pytest
import torch

import fsd_sample_ref as R1
import fsdv2_sample_ref as R
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAMES = ('seg_points', 'seg_logits', 'seg_vote_preds', 'seg_feats', 'center_preds', 'batch_idx')


def _build(config, **train_cfg):
    import sst_amd
    model = ast.literal_eval(open(os.path.join(GOLDEN, 'configs', 'fsdv2', f'{config}.model.py')).read())
    model['train_cfg'].update(train_cfg)
    torch.manual_seed(0)
    det = sst_amd.attach_fsdv2_heads(sst_amd.build_detector(model)).to(DEV)
    det.runtime_info = dict(enable_detection=True)       # past the pre-training phase: thresholds, not top-k
    return det


def _scene(box_cols):
    import bench_workloads as BW
    clouds = [BW.chain_cloud(2000, 5, half_extent=12.0).to(DEV), BW.chain_cloud(1900, 6, half_extent=12.0).to(DEV)]
    boxes, labels = [], []
    for s, cloud in enumerate(clouds):
        centre = cloud[[len(cloud) - 1, len(cloud) - 300, len(cloud) - 700], :3].cpu()
        b = torch.zeros(3, box_cols)
        b[:, :2], b[:, 2] = centre[:, :2], centre[:, 2] - 0.8
        b[:, 3:6], b[:, 6] = torch.tensor([1.6, 3.0, 1.6]), torch.tensor([0.3, -1.0, 2.0]) + s
        boxes.append(b.to(DEV))
        labels.append(torch.tensor([0, 1, 2], device=DEV))
    return clouds, boxes, labels


def _grouped(det):
    return bool(det.cfg.get('batched_group_sample', False))


def _thresholds(det, train):
    return R.thresholds32(det.cfg['score_thresh'], det.runtime_info.get('threshold_buffer', 0) if train else 0)


def _groups(det):
    return R.groups_by_names(det.cfg['group_names'], det.cfg['class_names'])


def _clear(det, logits, train):
    """bool [N]: every score of the row is clear of its threshold by the restatement's margin"""
    thr = _thresholds(det, train)
    if _grouped(det):
        return R.margin_ok(logits, _groups(det), thr).all(1)
    return R1.margin_ok(logits, thr).all(1)


def _calibrate(det, clouds, empty_last=None):
    """scale and bias the segmentation head's last layer so that every class (group) selects a share of the points strictly
    between none and all in the detector's current mode; rows whose score is ambiguous against a threshold get their last logit
    moved by 0.01 (both flows see the same logits); with ``empty_last`` that class (group) selects nothing in the last sample"""
    head = det.segmentor.segmentation_head
    head.__dict__.pop('forward', None)
    thr = torch.tensor(_thresholds(det, False), device=DEV)
    with torch.no_grad():
        spread = 2.0 / det.segmentor([c.clone() for c in clouds])['seg_logits'].std(0)     # logits of standard deviation 2
        head.conv_seg.weight.mul_(spread[:, None])
        head.conv_seg.bias.mul_(spread)
        logits = det.segmentor([c.clone() for c in clouds])['seg_logits']
        if _grouped(det):
            head.conv_seg.bias.add_(-torch.quantile(logits, 0.5, dim=0))
            head.conv_seg.bias[-1] += 1.0
            share = (R.grouped_scores(det.segmentor([c.clone() for c in clouds])['seg_logits'], _groups(det)) > thr[None]).float().mean(0)
        else:
            head.conv_seg.bias.add_(torch.log(thr / (1 - thr)) - torch.quantile(logits, 0.7, dim=0))
            share = (det.segmentor([c.clone() for c in clouds])['seg_logits'].sigmoid() > thr[None]).float().mean(0)
    assert bool(((share > 0.02) & (share < 0.9)).all()), share
    n0, plain = len(clouds[0]), type(head).forward
    cols = None if empty_last is None else (_groups(det)[empty_last] if _grouped(det) else [empty_last])

    def forward(voxel_feat):
        logits, votes = plain(head, voxel_feat)
        if cols is not None:
            logits = logits.clone()
            logits[n0:, cols] = -50.0
        for _ in range(4):
            if _grouped(det):                                # the background logit moves every score of the row
                bump = torch.zeros_like(logits)
                bump[:, -1] = 0.01
                logits = logits + bump * ~_clear(det, logits.detach(), det.training)[:, None]
            else:                                            # the ambiguous logit itself
                logits = logits + 0.01 * ~R1.margin_ok(logits.detach(), _thresholds(det, det.training))
        return logits, votes
    head.forward = forward


def _stage_by_indexing(det, seg_out, seg_feats, boxes, labels, train):
    """the stage between the segmentor and the head through the restatements -> (dict_to_sample, sampled, extracted, outs)"""
    det_ = (lambda t: t.detach()) if train else (lambda t: t)
    d = dict(seg_points=seg_out['seg_points'], seg_logits=det_(seg_out['seg_logits']), seg_vote_preds=det_(seg_out['seg_vote_preds']),
             seg_feats=seg_feats, batch_idx=seg_out['batch_idx'], vote_offsets=det_(seg_out['offsets']))
    thr = _thresholds(det, train)
    assert bool(_clear(det, d['seg_logits'], train).all()), 'a logit of this scene is ambiguous against its threshold'
    topk = train and det.train_cfg.get('disable_pretrain', False) and not det.runtime_info.get('enable_detection', False)
    if _grouped(det):
        groups = _groups(det)
        extra = R.topk_extra_mask(d['seg_logits'], groups, det.train_cfg['disable_pretrain_topks']) if topk else None
        smp = R.group_sample(d, groups, [float('inf')] * len(groups) if topk else thr, det.cfg.get('offset_scale', 1), extra)
    else:
        extra = R1.topk_extra_mask(d['seg_logits'], det.train_cfg['disable_pretrain_topks']) if topk else None
        smp = R1.sample(d, [float('inf')] * len(thr) if topk else thr, extra)
    share = torch.stack(smp['fg_mask_list']).float().mean(1)
    assert bool(((share > 0) & (share < 1)).all()), share
    comb = {k: torch.cat(smp[k], 0) for k in NAMES}
    ms_feats = seg_out['decoder_features']
    if train and det.train_cfg.get('detach_segmentor', False):
        ms_feats = [t.replace_feature(t.features.detach()) for t in ms_feats]
    ext = det.extract_feat(comb, dict(d, batch_size=int(d['batch_idx'].max()) + 1), gt_bboxes_3d=boxes, multiscale_features=ms_feats)
    outs = det.bbox_head(ext['virtual_feats'])
    return d, smp, ext, outs


def _second_stage_by_indexing(det, ext):
    """two_stage_fsd_v2.py:95-106: the boolean mask, the detector's own segmented means, the stable sort"""
    xyz, feats, bidx = ext['pts_xyz'], ext['pts_feats'], ext['pts_batch_inds']
    if not det.with_virtual:
        ori = ext['pts_indicators'] == 0
        xyz, feats, bidx = xyz[ori], feats[ori], bidx[ori]
    xyz, feats, bidx = det.pre_voxelize(xyz, feats, bidx)
    bidx, inds = torch.sort(bidx, stable=True)
    return xyz[inds], feats[inds], bidx


def _train_by_indexing(det, clouds, boxes, labels):
    metas = [{} for _ in clouds]
    seg_out = det.segmentor.forward_train(points=[c.clone() for c in clouds], img_metas=None, gt_bboxes_3d=boxes,
                                          gt_labels_3d=labels, as_subsegmentor=True)
    seg_feats = seg_out['seg_feats'].detach() if det.train_cfg.get('detach_segmentor', False) else seg_out['seg_feats']
    losses = dict(seg_out['losses'])
    d, smp, ext, outs = _stage_by_indexing(det, seg_out, seg_feats, boxes, labels, True)
    losses.update(det.bbox_head.loss(outs['cls_logits'], outs['reg_preds'], ext['virtual_centers'], ext['virtual_coors'][:, 0].contiguous(), boxes,
                                     labels, metas, iou_logits=outs.get('iou_logits', None), aux_xyz=ext['virtual_centroid']))
    losses['num_virtual'] = torch.ones(1, device=DEV) * ext['virtual_feats'].size(0)
    if hasattr(det, 'roi_head'):
        proposals = det.bbox_head.get_bboxes(outs['cls_logits'], outs['reg_preds'], ext['virtual_centers'], ext['virtual_coors'][:, 0],
                                             metas)
        losses.update(det.roi_head.forward_train(*_second_stage_by_indexing(det, ext), metas, proposals, boxes, labels))
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


@pytest.mark.parametrize('config,empty_last,pretrain', [('fsdv2_waymo_1x', None, False), ('fsdv2_nusc_1x', None, False),
                                                          ('fsdv2_nusc_1x', 3, False), ('fsdv2_waymo_1x', 2, False),
                                                          ('fsdv2_nusc_1x', None, True)])
def test_forward_train(config, empty_last, pretrain):
    import sst_amd
    det = _build(config).train()
    if pretrain:                                             # disable_pretrain before enable_detection: the top-k state
        det.runtime_info = {}
    assert type(det) is (sst_amd.FSDV2Step if config == 'fsdv2_waymo_1x' else sst_amd.SingleStageFSDV2Step)
    clouds, boxes, labels = _scene(7 if config == 'fsdv2_waymo_1x' else 9)
    _calibrate(det, clouds, empty_last)
    torch.manual_seed(1)
    losses = det.forward_train([c.clone() for c in clouds], [{} for _ in clouds], boxes, labels)
    assert {'loss_sem_seg', 'loss_vote', 'num_virtual'} <= set(losses) and any(k.startswith('loss_cls.task') for k in losses)
    if config == 'fsdv2_waymo_1x':
        assert {'loss_rcnn_cls', 'loss_rcnn_bbox'} <= set(losses)
    _total(losses).backward()
    got_grads = {n: p.grad.clone() for n, p in det.named_parameters() if p.grad is not None}
    det.zero_grad(set_to_none=True)
    det.print_info.clear()
    torch.manual_seed(1)
    want, smp = _train_by_indexing(det, clouds, boxes, labels)
    if empty_last is not None:
        assert smp['rule'][empty_last] and sum(smp['rule']) == 1, 'it selects nothing in the last sample: the rule gives it a point per sample'
    else:
        assert not any(smp['rule'])
    _same_losses(losses, want)
    _total(want).backward()
    for name, p in det.named_parameters():
        if p.grad is not None:
            assert name in got_grads and bool(torch.isfinite(got_grads[name]).all()), name
    for prefix in ('virtual_proj.', 'segmentor.backbone.', 'bbox_head.'):
        assert any(n.startswith(prefix) and float(g.abs().max()) > 0 for n, g in got_grads.items()), prefix


def test_detach_segmentor():
    """with train_cfg.detach_segmentor the segmentor's gradients are those of its own losses alone"""
    det = _build('fsdv2_nusc_1x', detach_segmentor=True).train()
    clouds, boxes, labels = _scene(9)
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


def test_simple_test_two_stage():
    det = _build('fsdv2_waymo_1x').eval()
    clouds, _, _ = _scene(7)
    clouds = clouds[:1]
    _calibrate(det, clouds)
    with torch.no_grad():
        metas = [{}]
        got = det.simple_test([c.clone() for c in clouds], metas)
        seg_out = det.segmentor.simple_test([c.clone() for c in clouds], metas)
        d, smp, ext, outs = _stage_by_indexing(det, seg_out, seg_out['seg_feats'], None, None, False)
        proposals = det.bbox_head.get_bboxes(outs['cls_logits'], outs['reg_preds'], ext['virtual_centers'], ext['virtual_coors'][:, 0],
                                             metas)
        want = det.roi_head.simple_test(*_second_stage_by_indexing(det, ext), metas, proposals, None, None)
        _same_boxes(got, want)
        det.test_cfg['skip_rcnn'] = True
        skipped = det.simple_test([c.clone() for c in clouds], metas)
    assert len(skipped) == 1 and set(skipped[0]) == {'boxes_3d', 'scores_3d', 'labels_3d'}
    pb = getattr(proposals[0][0], 'tensor', proposals[0][0])
    sb = getattr(skipped[0]['boxes_3d'], 'tensor', skipped[0]['boxes_3d'])
    assert pb.size(0) > 0 and torch.equal(sb, pb.cpu()) and torch.equal(skipped[0]['scores_3d'], proposals[0][1].cpu())
    assert torch.equal(skipped[0]['labels_3d'], proposals[0][2].cpu())


def test_simple_test_single_stage():
    det = _build('fsdv2_nusc_1x').eval()
    clouds, _, _ = _scene(9)
    _calibrate(det, clouds)
    with torch.no_grad():
        metas = [{} for _ in clouds]
        got = det.simple_test([c.clone() for c in clouds], metas)
        seg_out = det.segmentor.simple_test([c.clone() for c in clouds], metas)
        d, smp, ext, outs = _stage_by_indexing(det, seg_out, seg_out['seg_feats'], None, None, False)
        want = det.bbox_head.get_bboxes(outs['cls_logits'], outs['reg_preds'], ext['virtual_centers'], ext['virtual_coors'][:, 0], metas)
    assert len(got) == len(want) == 2 and sum(w[0].size(0) for w in want) > 0
    for g, w in zip(got, want):
        wb = getattr(w[0], 'tensor', w[0])
        gb = getattr(g['boxes_3d'], 'tensor', g['boxes_3d'])
        assert torch.equal(gb, wb.cpu()) and torch.equal(g['scores_3d'], w[1].cpu()) and torch.equal(g['labels_3d'], w[2].cpu())


def _g(array):
    return torch.from_numpy(np.ascontiguousarray(array))      # the file stores its matrices column-major


@pytest.mark.parametrize('with_virtual', [False, True])
@pytest.mark.parametrize('voxel', [None, (0.5, 0.5, 0.5)])
def test_second_stage_input_against_the_golden(with_virtual, voxel):
    """FSDV2Step.second_stage_input (the slice, one grouping and segmented means, the skipped or stable sort) against the
    reference's flow: rows and batch indices equal, the means within 1e-5 (the bar for segmented means; the fixture's sums are
    exact, so only the division rounds)"""
    gold = load_golden('fsdv2_sample.npz')
    det = _build('fsdv2_waymo_1x').eval()
    det.with_virtual = with_virtual
    det.test_cfg = dict(det.test_cfg, pre_2nd_voxelization=voxel)
    det.point_cloud_range = [float(x) for x in gold['ss_pc_range']]
    ind = _g(gold['ss_pts_indicators'])
    rpn = dict(pts_xyz=_g(gold['ss_pts_xyz']).to(DEV), pts_feats=_g(gold['ss_pts_feats']).to(DEV),
               pts_batch_inds=_g(gold['ss_pts_batch_inds']).to(DEV), pts_indicators=ind.to(DEV), num_ori_pts=int((ind == 0).sum()))
    xyz, feats, bidx = det.second_stage_input(rpn)
    tag = f'ss_v{int(with_virtual)}_p{int(voxel is not None)}'
    assert torch.equal(bidx.cpu(), _g(gold[f'{tag}_batch']))
    for got, key in ((xyz, 'xyz'), (feats, 'feats')):
        want = _g(gold[f'{tag}_{key}'])
        assert got.shape == want.shape and float((got.cpu() - want).abs().max()) < 1e-5, (tag, key)
    if voxel is None:
        assert torch.equal(xyz.cpu(), _g(gold[f'{tag}_xyz'])) and torch.equal(feats.cpu(), _g(gold[f'{tag}_feats'])), 'rows are only moved'
