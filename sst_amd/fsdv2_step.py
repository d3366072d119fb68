"""The FSDv2 detectors' training and test steps: ``attach_fsdv2_heads(det)`` builds the heads a freshly built
``SingleStageFSDV2`` / ``FSDV2`` parks in ``unbuilt`` and rebinds the instance to ``SingleStageFSDV2Step`` / ``FSDV2Step``, which
add ``sample``, ``combine_classes``, ``forward_train`` and ``simple_test`` over the sampling kernels
(``sst_amd.fg_sample`` for the per-class sigmoid path of the Waymo configs, ``sst_amd.fg_group_sample`` for
``batched_group_sample`` / ``group_sample`` of the nuScenes and Argoverse ones).  A detector built without the call is what it
was: no ``forward_train`` attribute, ``attach_heads()`` refusing by name.

Reference: mmdet3d/models/detectors/single_stage_fsd_v2.py:438-594 (forward_train, combine_classes, simple_test), :601-891
(sample, get_fg_mask, group_sample, batched_group_sample, get_offset_weight, gather_group_by_names);
two_stage_fsd_v2.py:62-199 (forward_train, simple_test, pre_voxelize).

Dropped: the reference's debugging asserts that read the device - ``(seg_logits < 0).any()`` (:612, :733), the ``isclose`` on
the offset weights (:771, :836), ``scores >= 0`` (:866, :882).  Refused by name: ``centroid_alpha``, ``baseline_mode``, an
``offset_weight`` other than ``'max'`` (as the reference), ``add_gt_fg_points`` on the grouped path (the reference cannot run
it there: it hands ``None`` boxes to get_fg_mask), ``aug_test``.  One difference in behaviour: ``train_cfg.detach_segmentor`` also
detaches the multi-scale decoder features, so that the segmentor's gradients are those of its own losses (the reference detaches
``seg_feats`` only; no shipped config sets the switch)."""
import torch

from . import fg_group_sample as GS
from . import fg_sample as FS
from . import kernels as K
from ._head_common import cfg_get as _get
from .detectors import FSDV2, SingleStageFSDV2, bbox3d2result, build_head
from .sst_ops import scatter_v2, unique_with_plan


class SingleStageFSDV2Step(SingleStageFSDV2):
    """``SingleStageFSDV2`` with its heads built and the steps of single_stage_fsd_v2.py:438-891.  Not registered: instances come
    from ``attach_fsdv2_heads``."""

    # ------------------------------------------------------------------------------------------------------------ sampling
    def _grouped(self):
        return bool(_get(self.cfg, 'group_sample', False) or _get(self.cfg, 'batched_group_sample', False))

    def _num_samples(self, batch_idx, batch_size=None):
        if batch_size is None:
            batch_size = getattr(self, '_batch_size', None)
        if batch_size is None:                           # called outside forward_train / simple_test: one read, as the reference
            batch_size = int(batch_idx[-1].item()) + 1 if batch_idx.numel() else 1
        return batch_size

    def _groups(self):
        cfg = self.train_cfg if self.training else self.test_cfg
        if _get(self.cfg, 'offset_weight', 'max') != 'max':
            raise NotImplementedError(f"SingleStageFSDV2.get_offset_weight: offset_weight {self.cfg['offset_weight']!r} (only 'max', "
                                      'as in the reference)')
        groups = GS.groups_by_names(cfg['group_names'], cfg['class_names'])
        if len(groups) != len(cfg['score_thresh']):
            raise RuntimeError(f"{len(groups)} groups for {len(cfg['score_thresh'])} score thresholds")
        return cfg, groups

    def _fg_inputs(self, seg_logits, seg_points, batch_idx, gt_bboxes_3d, gt_labels_3d, groups=None):
        """what get_fg_mask decides per class or group (:662-705) as the kernels' inputs: (float32 thresholds, extra mask)"""
        cfg = self.train_cfg if self.training else self.test_cfg
        n_cls, extra = (self.num_classes if groups is None else len(groups)), None
        if self.training and _get(self.train_cfg, 'disable_pretrain', False) and not self.runtime_info.get('enable_detection', False):
            topks = _get(self.train_cfg, 'disable_pretrain_topks', [100, 100, 100])
            thr = [float('inf')] * n_cls                 # the top-k indices replace the threshold
            extra = FS.topk_extra_mask(seg_logits, topks) if groups is None else GS.group_topk_extra_mask(seg_logits, groups, topks)
        else:
            buffer_thr = self.runtime_info.get('threshold_buffer', 0) if (self.training and self.runtime_info is not None) else 0
            thr = FS.round_thresholds(list(self.cfg['score_thresh'])[:n_cls], buffer_thr)
        if _get(cfg, 'add_gt_fg_points', False) and self.training and not self.runtime_info.get('stop_add_gt_fg_points', False):
            if groups is not None:
                raise NotImplementedError('SingleStageFSDV2.sample: add_gt_fg_points with group_sample / batched_group_sample (the '
                                          'reference passes no boxes to get_fg_mask there and cannot run it)')
            extra = FS.gt_extra_mask(seg_points, batch_idx, gt_bboxes_3d, gt_labels_3d, n_cls, out=extra)
        return thr, extra

    def get_fg_mask(self, seg_scores, seg_points, cls_id, batch_inds, gt_bboxes_3d, gt_labels_3d, seg_logits=None):
        """single_stage_fsd_v2.py:662-705 for one class (or group, on the grouped path), without the at-least-one-point rule, as
        there.  The kernels decide on the LOGITS: pass them as ``seg_logits`` (``seg_scores`` is not read)."""
        if seg_logits is None:
            raise NotImplementedError('get_fg_mask: pass seg_logits= (the kernel decides on the logits; scores alone are not enough)')
        if self._grouped():
            cfg, groups = self._groups()
            thr, extra = self._fg_inputs(seg_logits, seg_points, batch_inds, gt_bboxes_3d, gt_labels_3d, groups)
            votes = seg_logits.new_zeros((seg_logits.size(0), 3 * seg_logits.size(1)))
            pend = GS.group_sample_launch(seg_logits, votes, seg_points, batch_inds, groups, thr, self._num_samples(batch_inds),
                                          extra_mask=extra, apply_rule=False)
        else:
            thr, extra = self._fg_inputs(seg_logits, seg_points, batch_inds, gt_bboxes_3d, gt_labels_3d)
            pend = FS.fg_sample_launch(seg_logits, None, seg_points, batch_inds, thr, self._num_samples(batch_inds), extra,
                                       apply_rule=False)
        return pend.mask[cls_id]

    def sample(self, dict_to_sample, offset, gt_bboxes_3d=None, gt_labels_3d=None, batch_size=None):
        """single_stage_fsd_v2.py:601-654 (per-class sigmoid scores, over ``fg_sample``) and :726-853 (``group_sample`` /
        ``batched_group_sample``, over ``group_sample``): the reference's lists per class or group ``seg_points``, ``batch_idx``,
        ``center_preds``, ``fg_mask_list`` (+ ``src``, ``slot``, ``class_offsets``, ``totals``, ``rule``).  The wide tensors are
        NOT copied per class: ``combined`` holds the rows of all classes as ``extract_feat`` wants them (``virtual_input``, the
        clipped ``center_preds``, ``seg_points``, ``batch_idx``), written by one gather.  One host read."""
        seg_logits, seg_points, batch_idx = dict_to_sample['seg_logits'], dict_to_sample['seg_points'], dict_to_sample['batch_idx']
        width = seg_logits.size(1)
        if self._grouped():
            if width != self.num_classes + 1:
                raise NotImplementedError(f'SingleStageFSDV2.sample: group_sample needs seg_logits with {self.num_classes} class '
                                          f'columns and the background ({self.num_classes + 1}), got {width}')
            cfg, groups = self._groups()
            thr, extra = self._fg_inputs(seg_logits, seg_points, batch_idx, gt_bboxes_3d, gt_labels_3d, groups)
            batched = bool(_get(self.cfg, 'batched_group_sample', False)) and not _get(self.cfg, 'group_sample', False)
            n_samples = self._num_samples(batch_idx, batch_size)
            if not batched and n_samples != 1:
                raise NotImplementedError('SingleStageFSDV2.group_sample: one sample only, as in the reference (:728); '
                                          'batched_group_sample takes a batch')
            scale = _get(cfg, 'offset_scale', 1) if batched else 1
            out = dict(GS.group_sample(seg_logits, offset, seg_points, batch_idx, groups, thr, n_samples, scale, extra))
        elif width == self.num_classes:
            thr, extra = self._fg_inputs(seg_logits, seg_points, batch_idx, gt_bboxes_3d, gt_labels_3d)
            out = dict(FS.fg_sample(seg_logits, offset, seg_points, batch_idx, thr, self._num_samples(batch_idx, batch_size), extra))
        else:
            raise NotImplementedError(f'SingleStageFSDV2.sample: seg_logits of width {width} fits neither the per-class sigmoid path '
                                      f'({self.num_classes} columns) nor group_sample / batched_group_sample '
                                      f'({self.num_classes + 1} columns and the config switch)')
        rows, clipped = GS.virtual_rows(out, dict_to_sample['seg_feats'], seg_logits, seg_points, self.point_cloud_range)
        out['combined'] = dict(seg_points=out['points_cat'], batch_idx=out['batch_cat'], center_preds=clipped, virtual_input=rows)
        out['source'] = dict_to_sample
        return out

    def combine_classes(self, data_dict, name_list):
        """single_stage_fsd_v2.py:508-513.  A dictionary ``sample`` made carries the classes combined already (``combined``):
        those are handed out - ``virtual_input`` in place of ``seg_feats`` / ``seg_logits``, which ``extract_feat`` would only
        concatenate again.  Any other dictionary of per-class lists is concatenated as the reference does."""
        done = data_dict.get('combined') if isinstance(data_dict, dict) else None
        if done is not None:
            return dict(done)
        return {name: torch.cat(data_dict[name], 0) for name in data_dict if name in name_list}

    # --------------------------------------------------------------------------------------------------------------- steps
    def _stage(self, seg_out_dict, seg_feats, gt_bboxes_3d, gt_labels_3d, train):
        """what forward_train (:461-480) and simple_test (:554-572) share between the segmentor and the box head"""
        det = (lambda t: t.detach()) if train else (lambda t: t)
        dict_to_sample = dict(seg_points=seg_out_dict['seg_points'], seg_logits=det(seg_out_dict['seg_logits']),
                              seg_vote_preds=det(seg_out_dict['seg_vote_preds']), seg_feats=seg_feats,
                              batch_idx=seg_out_dict['batch_idx'], vote_offsets=det(seg_out_dict['offsets']))
        sampled_out = self.sample(dict_to_sample, dict_to_sample['vote_offsets'], gt_bboxes_3d, gt_labels_3d)
        combined_out = self.combine_classes(sampled_out, ['seg_points', 'seg_logits', 'seg_vote_preds', 'seg_feats', 'center_preds',
                                                          'batch_idx'])
        origin = dict(dict_to_sample, batch_size=self._batch_size)
        ms_feats = seg_out_dict['decoder_features']
        if train and ms_feats is not None and _get(self.train_cfg, 'detach_segmentor', False):
            # the reference detaches seg_feats alone (:456-457), which leaves the multi-scale decoder features as a second way
            # into the segmentor; here detach_segmentor closes both (no shipped config sets it)
            ms_feats = [t.replace_feature(t.features.detach()) for t in ms_feats]
        extract_output = self.extract_feat(combined_out, origin, gt_bboxes_3d=gt_bboxes_3d, multiscale_features=ms_feats)
        outs = self.bbox_head(extract_output['virtual_feats'])
        return dict_to_sample, sampled_out, extract_output, outs

    def forward_train(self, points, img_metas, gt_bboxes_3d, gt_labels_3d, gt_bboxes_ignore=None, runtime_info=None):
        """single_stage_fsd_v2.py:438-505: points and ground-truth boxes -> the loss dictionary (segmentor losses, the head's
        losses with ``aux_xyz = virtual_centroid`` for ``centroid_assign``, ``num_virtual``), or with ``as_rpn`` the reference's
        output dictionary for the RoI stage (+ ``num_ori_pts``: how many of the ``pts_*`` rows are original points)."""
        if runtime_info is not None:
            self.runtime_info = runtime_info
        losses = {}
        gt_bboxes_3d = [b[l >= 0] for b, l in zip(gt_bboxes_3d, gt_labels_3d)]
        gt_labels_3d = [l[l >= 0] for l in gt_labels_3d]
        self._batch_size = len(points)
        seg_out_dict = self.segmentor.forward_train(points=points, img_metas=img_metas, gt_bboxes_3d=gt_bboxes_3d,
                                                    gt_labels_3d=gt_labels_3d, as_subsegmentor=True)
        seg_feats = seg_out_dict['seg_feats']
        if _get(self.train_cfg, 'detach_segmentor', False):
            seg_feats = seg_feats.detach()
        losses.update(seg_out_dict['losses'])
        dict_to_sample, _, extract_output, outs = self._stage(seg_out_dict, seg_feats, gt_bboxes_3d, gt_labels_3d, True)
        voxel_xyz, voxel_coors = extract_output['virtual_centers'], extract_output['virtual_coors']
        det_loss = self.bbox_head.loss(outs['cls_logits'], outs['reg_preds'], voxel_xyz, voxel_coors[:, 0].contiguous(), gt_bboxes_3d,
                                       gt_labels_3d, img_metas, iou_logits=outs.get('iou_logits', None),
                                       gt_bboxes_ignore=gt_bboxes_ignore, aux_xyz=extract_output['virtual_centroid'])
        if hasattr(self.bbox_head, 'print_info'):
            self.print_info.update(self.bbox_head.print_info)
        losses.update(det_loss)
        losses.update(self.print_info)
        if not self.as_rpn:
            return losses
        return dict(rpn_losses=losses, cls_logits=outs['cls_logits'], reg_preds=outs['reg_preds'], voxel_xyz=voxel_xyz,
                    voxel_batch_inds=voxel_coors[:, 0], pts_feats=extract_output['pts_feats'], pts_xyz=extract_output['pts_xyz'],
                    pts_indicators=extract_output['pts_indicators'], pts_batch_inds=extract_output['pts_batch_inds'],
                    num_ori_pts=dict_to_sample['seg_points'].size(0))

    def simple_test(self, points, img_metas, imgs=None, rescale=False, gt_bboxes_3d=None, gt_labels_3d=None):
        """single_stage_fsd_v2.py:539-594"""
        if gt_bboxes_3d is not None:
            gt_bboxes_3d, gt_labels_3d = gt_bboxes_3d[0], gt_labels_3d[0]
            assert isinstance(gt_bboxes_3d, list) and isinstance(gt_labels_3d, list)
            assert len(gt_bboxes_3d) == len(gt_labels_3d) == 1, 'assuming single sample testing'
        self._batch_size = len(points)
        seg_out_dict = self.segmentor.simple_test(points, img_metas)
        dict_to_sample, _, extract_output, outs = self._stage(seg_out_dict, seg_out_dict['seg_feats'], gt_bboxes_3d, gt_labels_3d,
                                                              False)
        bbox_list = self.bbox_head.get_bboxes(outs['cls_logits'], outs['reg_preds'], extract_output['virtual_centers'],
                                              extract_output['virtual_coors'][:, 0], img_metas, rescale=rescale,
                                              iou_logits=outs.get('iou_logits', None))
        if self.as_rpn:
            return dict(pts_feats=extract_output['pts_feats'], pts_xyz=extract_output['pts_xyz'],
                        pts_indicators=extract_output['pts_indicators'], pts_batch_inds=extract_output['pts_batch_inds'],
                        proposal_list=bbox_list, num_ori_pts=dict_to_sample['seg_points'].size(0))
        return [bbox3d2result(bboxes, scores, labels) for bboxes, scores, labels in bbox_list]

    def aug_test(self, points, img_metas, imgs=None, rescale=False):
        raise NotImplementedError('SingleStageFSDV2.aug_test is not built (the reference returns NotImplementedError)')


class FSDV2Step(SingleStageFSDV2Step, FSDV2):
    """``FSDV2`` with both heads built and the steps of two_stage_fsd_v2.py:62-199"""

    def second_stage_input(self, rpn_outs):
        """two_stage_fsd_v2.py:90-106: the points the RoI head sees.  ``pts_indicators == 0`` selects exactly the first
        ``num_ori_pts`` rows of what ``extract_feat`` returns (original points, then voted centres), so it is a slice: no mask,
        no host read.  After ``pre_voxelize`` the batch indices come from a sorted-unique and after the slice from the
        segmentor's non-decreasing ``batch_idx``: the reference's ``sort()`` is the identity there and is skipped.  Only
        ``with_virtual`` without a second voxelization concatenates two sorted runs; that is sorted stably (the reference's
        ``sort()`` leaves the order inside a sample open on a GPU)."""
        pts_xyz, pts_feats, pts_batch_inds = rpn_outs['pts_xyz'], rpn_outs['pts_feats'], rpn_outs['pts_batch_inds']
        if not self.with_virtual:
            n_ori = rpn_outs['num_ori_pts']
            pts_xyz, pts_feats, pts_batch_inds = pts_xyz[:n_ori], pts_feats[:n_ori], pts_batch_inds[:n_ori]
        cfg = self.train_cfg if self.training else self.test_cfg
        if _get(cfg, 'pre_2nd_voxelization', None) is not None:
            return self.pre_voxelize(pts_xyz, pts_feats, pts_batch_inds)
        if self.with_virtual:
            pts_batch_inds, inds = torch.sort(pts_batch_inds, stable=True)
            pts_xyz, pts_feats = pts_xyz[inds], pts_feats[inds]
        return pts_xyz, pts_feats, pts_batch_inds

    def pre_voxelize(self, points, features, batch_idx):
        """two_stage_fsd_v2.py:172-199: one grouping (``unique_with_plan``), one segmented mean per tensor over its plan"""
        cfg = self.train_cfg if self.training else self.test_cfg
        voxel_size = _get(cfg, 'pre_2nd_voxelization', None)
        if voxel_size is None:
            return points, features, batch_idx
        vs = K.const_tensor(voxel_size, points.device)
        lo = K.const_tensor(self.point_cloud_range[:3], points.device)
        coors = torch.div(points[:, :3] - lo[None], vs[None], rounding_mode='floor').long()[:, [2, 1, 0]]
        coors = torch.cat([batch_idx.long()[:, None], coors], dim=1)
        new_coors, unq_inv = unique_with_plan(coors)
        new_points = scatter_v2(points, coors, mode='avg', return_inv=False, new_coors=new_coors, unq_inv=unq_inv)[0]
        new_feats = scatter_v2(features, coors, mode='avg', return_inv=False, new_coors=new_coors, unq_inv=unq_inv)[0]
        return new_points, new_feats, new_coors[:, 0]

    def forward_train(self, points, img_metas, gt_bboxes_3d, gt_labels_3d, gt_bboxes_ignore=None):
        """two_stage_fsd_v2.py:62-120: the first stage as RPN, its boxes as proposals, the RoI head's losses"""
        gt_bboxes_3d = [b[l >= 0] for b, l in zip(gt_bboxes_3d, gt_labels_3d)]
        gt_labels_3d = [l[l >= 0] for l in gt_labels_3d]
        losses = {}
        rpn_outs = super().forward_train(points=points, img_metas=img_metas, gt_bboxes_3d=gt_bboxes_3d, gt_labels_3d=gt_labels_3d,
                                         gt_bboxes_ignore=gt_bboxes_ignore, runtime_info=self.runtime_info)
        losses.update(rpn_outs['rpn_losses'])
        proposal_list = self.bbox_head.get_bboxes(rpn_outs['cls_logits'], rpn_outs['reg_preds'], rpn_outs['voxel_xyz'],
                                                  rpn_outs['voxel_batch_inds'], img_metas)
        assert len(proposal_list) == len(gt_bboxes_3d)
        pts_xyz, pts_feats, pts_batch_inds = self.second_stage_input(rpn_outs)
        losses.update(self.roi_head.forward_train(pts_xyz, pts_feats, pts_batch_inds, img_metas, proposal_list, gt_bboxes_3d,
                                                  gt_labels_3d))
        return losses

    def simple_test(self, points, img_metas, imgs=None, rescale=False, gt_bboxes_3d=None, gt_labels_3d=None):
        """two_stage_fsd_v2.py:122-169"""
        rpn_outs = super().simple_test(points=points, img_metas=img_metas, gt_bboxes_3d=gt_bboxes_3d, gt_labels_3d=gt_labels_3d)
        proposal_list = rpn_outs['proposal_list']
        if _get(self.test_cfg, 'skip_rcnn', False):
            return [bbox3d2result(bboxes, scores, labels) for bboxes, scores, labels in proposal_list]
        pts_xyz, pts_feats, pts_batch_inds = self.second_stage_input(rpn_outs)
        return self.roi_head.simple_test(pts_xyz, pts_feats, pts_batch_inds, img_metas, proposal_list, gt_bboxes_3d, gt_labels_3d)


def attach_fsdv2_heads(det):
    """Opt in to the FSDv2 training and test steps: build ``bbox_head`` (``FSDV2Head``) by the documented
    ``build_head(dict(det.unbuilt['bbox_head'], train_cfg=det.train_cfg, test_cfg=det.test_cfg))`` and, for ``FSDV2``,
    ``roi_head`` with the ``rcnn`` parts, as submodules, and rebind the instance to ``SingleStageFSDV2Step`` / ``FSDV2Step``.
    ``unbuilt`` and every ``state_dict`` key outside ``bbox_head.`` / ``roi_head.`` stay as they are.  -> det"""
    if isinstance(det, SingleStageFSDV2Step):
        return det
    if type(det) not in (SingleStageFSDV2, FSDV2):
        raise NotImplementedError(f'attach_fsdv2_heads: {type(det).__name__} is not an FSDv2 detector (SingleStageFSDV2 / FSDV2); '
                                  'the FSD ones have attach_heads()')
    cfg = det.unbuilt['bbox_head']
    if cfg.get('type') != 'FSDV2Head':
        raise NotImplementedError(f"attach_fsdv2_heads: bbox_head {cfg.get('type')} - the FSDv2 step is built over FSDV2Head")
    for part in (det.train_cfg, det.test_cfg):
        if _get(part, 'centroid_alpha', None) is not None:
            raise NotImplementedError('attach_fsdv2_heads: centroid_alpha is not built')
        if _get(part, 'baseline_mode', False):
            raise NotImplementedError('attach_fsdv2_heads: baseline_mode is not built')
        if _get(part, 'offset_weight', 'max') != 'max':
            raise NotImplementedError(f"attach_fsdv2_heads: offset_weight {_get(part, 'offset_weight')!r} (only 'max', as in the "
                                      'reference)')
    det.bbox_head = build_head(dict(cfg, train_cfg=det.train_cfg, test_cfg=det.test_cfg))
    if type(det) is FSDV2:
        roi = det.unbuilt['roi_head']
        det.roi_head = build_head(dict(roi, train_cfg=_get(det.train_cfg, 'rcnn', None), test_cfg=_get(det.test_cfg, 'rcnn', None)))
        det.__class__ = FSDV2Step
    else:
        det.__class__ = SingleStageFSDV2Step
    return det
