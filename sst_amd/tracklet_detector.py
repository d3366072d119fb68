"""The CTRL tracklet family's modules (configs/ctrl/ctrl_{veh,ped}_24e.py, ctrl_cyc_12e.py): TrackletPointRoIExtractor
(roi_heads/roi_extractors/dynamic_point_roi_extractor.py:147-295), TrackletRoIHead (roi_heads/tracklet_roi_head.py) with the
decoding of FullySparseBboxHead.get_bboxes_from_tracklet (bbox_heads/fsd_bbox_head.py:792-869) as a function, TimestampEncoder,
TrackletSegmentor and TrackletDetector (detectors/tracklet_detector.py).  Names, constructor arguments and return values are the
reference's.  The training step makes its targets in one launch (sst_amd.tracklet_targets) and the rows of the box head in one
launch (sst_amd.tracklet_rows); the one host read of a step is the point pool's pair count.

Refused by name (no shipped config sets them): merge_candidates, pre_voxelization_size, with_roi_corners, checkpointing, tta /
aug_test.  The dataset and the Tracklet* pipeline transforms are not part of this library.
"""
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from ._head_common import cfg_get as _cfg_get
from .detectors import DETECTORS, HEADS, build_detector, build_head, build_neck
from .dynamic_point_pool import DynamicPointROIExtractor, dynamic_point_pool_mixed
from .registry import ROI_EXTRACTORS, build_backbone, build_middle_encoder, build_voxel_encoder
from .roi_head import roi_decode
from .sst_ops import scatter_v2
from .tracklet import LiDARTracklet, aligned_iou_3d, tracklet_rows, tracklet_targets
from .voxel import Voxelization
from . import kernels as K


def _refuse(what):
    raise NotImplementedError(f'sst_amd: {what} is not built (no shipped CTRL config sets it)')


@ROI_EXTRACTORS.register_module()
class TrackletPointRoIExtractor(nn.Module):
    """The points of every RoI of every tracklet over the mixed point pool.  combined: a point pairs with every box of its
    tracklet (the sample index alone is compared); separate: only with the box of its own frame (sample x frame).
    max_all_point: a number, or (training, testing).  -> (point indices, RoI indices, dict(local_xyz, boundary_offset,
    is_in_margin)); a batch without any pair gives the pool's fake row (-1, -1, zeros)."""

    def __init__(self, init_cfg=None, debug=True, extra_wlh=[0, 0, 0], max_inbox_point=512, max_all_point=200000, combined=False):
        super().__init__()
        self.init_cfg = init_cfg
        self.debug = debug
        self.extra_wlh = extra_wlh
        self.max_inbox_point = max_inbox_point
        self.max_all_point = max_all_point
        self.combined = combined

    def _cap(self):
        if isinstance(self.max_all_point, (tuple, list)):
            return self.max_all_point[0] if self.training else self.max_all_point[1]
        return self.max_all_point

    def forward(self, pts_xyz, batch_inds, pts_frame_inds, rois, roi_frame_inds, max_inbox_point=None):
        assert len(pts_xyz) > 0
        assert len(batch_inds) > 0
        assert len(rois) > 0
        if self.combined:
            pts_inds, roi_inds = batch_inds, rois[:, 0]
        else:
            # one id per (sample, frame); the stride covers the frames of both sides, so that ids never collide (the reference
            # reads both maxima to the host and asserts the points' frames lie within the RoIs')
            max_frames = torch.maximum(roi_frame_inds.max(), pts_frame_inds.max()) + 1
            pts_inds = batch_inds * max_frames + pts_frame_inds
            roi_inds = rois[:, 0].int() * max_frames + roi_frame_inds
        pts_inds, roi_inds = pts_inds.int(), roi_inds.int()
        all_inds, all_roi_inds, info = dynamic_point_pool_mixed(rois[..., 1:8].contiguous(), roi_inds, pts_xyz, pts_inds, self.extra_wlh,
                                                                self.max_inbox_point, self._cap())
        if self.debug:
            self.check_invariants(pts_xyz, rois[..., 1:8], pts_inds, roi_inds, all_inds, all_roi_inds, info)
        return all_inds, all_roi_inds, dict(local_xyz=info[:, 3:6], boundary_offset=info[:, 6:-1], is_in_margin=info[:, -1])

    def check_invariants(self, pts_xyz, rois7, pts_inds, roi_inds, all_inds, all_roi_inds, info):
        """the reference's debug block (:217-229): the geometry of every pair, and every pair joins a point and a RoI of one id
        (its loop over the RoIs, as one comparison)"""
        DynamicPointROIExtractor.check_invariants(self, pts_xyz, rois7, all_inds, all_roi_inds, info[:, :3], info[:, 3:6], info[:, 6:-1])
        ok = all_inds >= 0
        assert (roi_inds[all_roi_inds[ok]] == pts_inds[all_inds[ok]]).all()
        if not self.combined:
            assert len(roi_inds) == len(torch.unique(roi_inds))


@torch.no_grad()
def decode_tracklet_rows(rois, cls_score, bbox_pred, class_pred, gt_rois=None, cfg=None):
    """the decoding of FullySparseBboxHead.get_bboxes_from_tracklet (fsd_bbox_head.py:792-869) before it is split by tracklet
    -> (boxes [R, 7], scores [R]): ``roi_decode``, or the RoIs and their scores under identical_decode; replace_center /
    replace_size / replace_yaw take the ground truth ``gt_rois`` [R, 8] = (valid, box) where it exists"""
    assert rois.size(0) == cls_score.size(0) == bbox_pred.size(0)
    if _cfg_get(cfg, 'identical_decode', False):
        boxes, scores = rois[:, 1:].clone(), class_pred
    else:
        boxes, scores, _ = roi_decode(rois.contiguous(), _lib.as_fp32(bbox_pred).contiguous(), _lib.as_fp32(cls_score).contiguous(),
                                      with_bev=False)
    for key, cols, gcols in (('replace_center', slice(0, 3), slice(1, 4)), ('replace_size', slice(3, 6), slice(4, 7)),
                             ('replace_yaw', slice(6, 7), slice(7, 8))):
        if _cfg_get(cfg, key, False):
            assert gt_rois is not None and gt_rois.size(1) == 8
            boxes[:, cols] = torch.where(gt_rois[:, 0:1].bool(), gt_rois[:, gcols].to(boxes.dtype), boxes[:, cols])
    return boxes, scores


@torch.no_grad()
def get_bboxes_from_tracklet(rois, cls_score, bbox_pred, valid_roi_mask, class_labels, class_pred, img_metas=None, gt_rois=None,
                             cfg=None, batch_size=None):
    """FullySparseBboxHead.get_bboxes_from_tracklet (fsd_bbox_head.py:792-869) over ``roi_decode``: per tracklet (boxes, scores,
    labels, valid mask), invalid RoIs left in (the tracklet keeps its old box there).  cfg: identical_decode (the RoIs and their
    scores pass through), replace_center / replace_size / replace_yaw (the ground truth ``gt_rois`` [R, 8] = (valid, box) where
    it exists).  batch_size: the number of tracklets (default: read from the RoIs, one host read as in the reference)."""
    boxes, scores = decode_tracklet_rows(rois, cls_score, bbox_pred, class_pred, gt_rois, cfg)
    roi_batch_id = rois[..., 0]
    if batch_size is None:
        batch_size = int(roi_batch_id.max().item() + 1)
    counts = torch.bincount(roi_batch_id.long(), minlength=batch_size).tolist() if batch_size > 1 else [rois.size(0)]
    result_list, r0 = [], 0
    for i, n in enumerate(counts):     # the RoIs of a tracklet are one run (tracklets2rois)
        sl = slice(r0, r0 + n)
        box_type = (img_metas[i] or {}).get('box_type_3d') if img_metas else None
        b = boxes[sl]
        result_list.append((box_type(b, b.size(1)) if box_type is not None else b, scores[sl].view(-1), class_labels[sl],
                            valid_roi_mask[sl]))
        r0 += n
    return result_list


@HEADS.register_module()
class TrackletRoIHead(nn.Module):
    """roi_heads/tracklet_roi_head.py: refines every box of every tracklet from the points of its tracklet."""

    def __init__(self, num_classes=3, roi_extractor=None, bbox_head=None, train_cfg=None, test_cfg=None, pretrained=None,
                 init_cfg=None, general_cfg=dict()):
        super().__init__()
        assert not (init_cfg and pretrained), 'init_cfg and pretrained cannot be setting at the same time'
        self.general_cfg = general_cfg
        self.num_classes = num_classes
        self.with_roi_scores = _cfg_get(general_cfg, 'with_roi_scores', False)
        if _cfg_get(general_cfg, 'with_roi_corners', False):
            _refuse('TrackletRoIHead: general_cfg with_roi_corners')
        if _cfg_get(general_cfg, 'checkpointing', False):
            _refuse('TrackletRoIHead: general_cfg checkpointing')
        if _cfg_get(train_cfg, 'merge_candidates', False):
            _refuse('TrackletRoIHead: train_cfg merge_candidates')
        if _cfg_get(test_cfg, 'tta', None) is not None:
            _refuse('TrackletRoIHead: test_cfg tta')
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.roi_extractor = ROI_EXTRACTORS.build(dict(roi_extractor))
        self.bbox_head = build_head(dict(bbox_head, train_cfg=train_cfg, test_cfg=test_cfg))
        if train_cfg is not None:
            assigner = dict(_cfg_get(train_cfg, 'assigner'))
            if assigner.pop('type', 'TrackletAssigner') != 'TrackletAssigner':
                raise NotImplementedError('TrackletRoIHead: only TrackletAssigner is built')
            self.assigner_cfg = assigner

    @property
    def with_bbox(self):
        return True

    def class_indices(self, tracklet_list):
        """the class of every tracklet: ``trk.type`` in the 'mmdet3d' format (WaymoTrackletDataset maps the type name to its
        position in class_names before the tracklets reach the head)"""
        assert all(t.type_format == 'mmdet3d' for t in tracklet_list), 'tracklet types must be class indices (set_type(i, "mmdet3d"))'
        return [int(t.type) for t in tracklet_list]

    def _assign_and_sample(self, tracklet_list, candidates_list):
        """-> the dict of ``tracklet_targets`` (candidate choice, assignment, PseudoSampler's order and the targets: one launch)"""
        assert len(tracklet_list) == len(candidates_list)
        return tracklet_targets(tracklet_list, candidates_list, self.train_cfg, assigner=self.assigner_cfg,
                                num_classes=max(self.num_classes, 1), class_indices=self.class_indices(tracklet_list))

    def _select_one2one_candidates(self, tracklet_list, candidates_list):
        """-> per tracklet its chosen candidate (an empty tracklet without one); one launch and one read of T integers"""
        chosen = self._assign_and_sample(tracklet_list, candidates_list)['chosen'].tolist()
        return [c[k] if k >= 0 else t.new_empty() for t, c, k in zip(tracklet_list, candidates_list, chosen)]

    def tracklets2rois(self, tracklets):
        """-> (rois [R, 8] = (tracklet, box), roi_frame_inds, cls_preds (the boxes' scores), labels_3d)"""
        dev = tracklets[0].device
        rois = torch.cat([F.pad(t.concated_boxes()[:, :7], (1, 0), value=float(i)) for i, t in enumerate(tracklets)], 0)
        cls_preds = torch.tensor([s for t in tracklets for s in t.score_list], dtype=torch.float).to(dev, non_blocking=True)
        labels_3d = torch.tensor([int(t.type) for t in tracklets for _ in range(len(t))], dtype=torch.long).to(dev, non_blocking=True)
        roi_frame_inds = torch.tensor([k for t in tracklets for k in range(len(t))], dtype=torch.long).to(dev, non_blocking=True)
        assert tracklets[0].type_format == 'mmdet3d'
        return rois, roi_frame_inds, cls_preds, labels_3d

    def get_gt_rois(self, tracklets, gt_tracklets):
        assert len(tracklets) == len(gt_tracklets)
        pairs = [gt.concated_boxes_from_ts(trk.ts_list) for trk, gt in zip(tracklets, gt_tracklets)]
        dev = tracklets[0].device
        gt_rois, mask = torch.cat([p[0].to(dev) for p in pairs], 0), torch.cat([p[1].to(dev) for p in pairs], 0)
        return torch.cat([mask[:, None].to(gt_rois.dtype), gt_rois], 1)

    def _bbox_forward(self, pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds, rois, roi_scores, roi_frame_inds):
        assert pts_xyz.size(0) == pts_feats.size(0) == pts_batch_idx.size(0) == pts_frame_inds.size(0)
        ext_pts_inds, ext_pts_roi_inds, ext_pts_info = self.roi_extractor(pts_xyz[:, :3], pts_batch_idx, pts_frame_inds,
                                                                          rois[:, :8].contiguous(), roi_frame_inds)
        new_pts_feats, new_pts_xyz = tracklet_rows(_lib.as_fp32(pts_feats), pts_xyz, pts_frame_inds, ext_pts_inds, ext_pts_roi_inds,
                                                   roi_frame_inds, roi_scores, combined=self.roi_extractor.combined,
                                                   with_roi_scores=self.with_roi_scores)
        cls_score, bbox_pred, valid_roi_mask = self.bbox_head(new_pts_xyz, new_pts_feats, ext_pts_info, ext_pts_roi_inds, rois)
        return dict(cls_score=cls_score, bbox_pred=bbox_pred, valid_roi_mask=valid_roi_mask)

    def _bbox_forward_train(self, pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds, targets):
        rois = targets['rois']
        res = self._bbox_forward(pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds, rois, targets['scores'], targets['frame_inds'])
        loss_bbox = self.bbox_head.loss(res['cls_score'], res['bbox_pred'], res['valid_roi_mask'], rois, targets)
        loss_bbox.update(self.iou_logs(rois, res['bbox_pred'], targets, pts_xyz))
        res.update(loss_bbox=loss_bbox)
        return res

    @torch.no_grad()
    def iou_logs(self, rois, bbox_pred, targets, pts_xyz):
        """refined_iou, roi_iou, num_good, num_good_rois (tracklet_roi_head.py:198-230) without a mask compaction: the aligned
        IoU of every row with its (zero off the positives) matched box, averaged over the positives on the device"""
        good_thresh = 0.7 if _cfg_get(self.train_cfg, 'class_names')[0] == 'Car' else 0.5
        pos = targets['reg_mask'] > 0
        n_pos = pos.sum()
        gt = torch.where(pos[:, None], targets['pos_gt_bboxes'], rois[:, 1:8])       # off the positives: any valid box
        decoded = self.bbox_head.decode_from_rois(rois, bbox_pred.detach())
        out = {}
        for name, good, boxes in (('refined_iou', 'num_good', decoded), ('roi_iou', 'num_good_rois', rois[:, 1:8].contiguous())):
            ious = aligned_iou_3d(gt.contiguous(), boxes[:, :7].contiguous())
            zero = torch.zeros_like(ious)
            mean = torch.where(pos, ious, zero).sum() / n_pos.clamp(min=1)
            count = (pos & (ious > good_thresh)).sum().float()
            # no positive at all: the reference logs 0.5 and 1
            out[name] = torch.where(n_pos > 0, mean, mean.new_full((), 0.5))
            out[good] = torch.where(n_pos > 0, count, count.new_ones(()))
        return out

    def forward_train(self, pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds, img_metas, tracklet_list, gt_candidates_list):
        targets = self._assign_and_sample(tracklet_list, gt_candidates_list)
        return dict(self._bbox_forward_train(pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds, targets)['loss_bbox'])

    @torch.no_grad()
    def simple_test(self, pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds, img_metas, tracklet_list, gt_candidates_list=None, **kwargs):
        """-> the tracklets, updated from the predictions (a row with an invalid RoI keeps its old box)"""
        gt_rois = None
        if gt_candidates_list is not None:
            gt_rois = self.get_gt_rois(tracklet_list, self._select_one2one_candidates(tracklet_list, gt_candidates_list))
        assert all(len(t) > 0 for t in tracklet_list), 'make sure there is no empty tracklet'
        rois, roi_frame_inds, cls_preds, labels_3d = self.tracklets2rois(tracklet_list)
        res = self._bbox_forward(pts_xyz, pts_feats, pts_batch_idx, pts_frame_inds, rois, cls_preds, roi_frame_inds)
        decoded = get_bboxes_from_tracklet(rois, res['cls_score'], res['bbox_pred'], res['valid_roi_mask'], labels_3d, cls_preds, None,
                                           gt_rois=gt_rois, cfg=self.test_cfg, batch_size=len(tracklet_list))
        assert len(decoded) == len(tracklet_list)
        for trk, (boxes, scores, labels, valid_mask) in zip(tracklet_list, decoded):
            trk.update_from_prediction(boxes, scores, labels, valid_mask)
        return list(tracklet_list)


class TimestampEncoder(nn.Module):
    """the frame time of a point as one more input column (tracklet_detector.py:458-481)"""

    def __init__(self, strategy_cfg):
        super().__init__()
        self.strategy_cfg = strategy_cfg
        if strategy_cfg['strategy'] != 'scalar':
            raise NotImplementedError(f'TimestampEncoder: strategy {strategy_cfg["strategy"]!r} (the reference has only \'scalar\')')

    def forward(self, point, pts_frame_inds):
        # the reference's three range asserts (point[:, -1] < 200, 0 <= pts_frame_inds <= 200) cost three host reads per step:
        # they guard the data pipeline, which is not part of this library
        return self.scalar(point, pts_frame_inds)

    def scalar(self, point, pts_frame_inds):
        n = self.strategy_cfg['normalizer']
        return torch.cat([point, point[:, -1:] / n], 1)


@DETECTORS.register_module()
class TrackletSegmentor(nn.Module):
    """the point feature extractor of the tracklet detector (tracklet_detector.py:22-187): dynamic voxelisation, the timestamp
    column, DynamicScatterVFE, the sparse U-Net and the voxel-to-point neck; no segmentation head in the shipped configs."""

    def __init__(self, voxel_layer, timestamp_encoder, voxel_encoder, middle_encoder, backbone, segmentation_head, decode_neck=None,
                 voxel_downsampling_size=None, train_cfg=None, test_cfg=None, init_cfg=None, pretrained=None, tanh_dims=None,
                 **extra_kwargs):
        super().__init__()
        assert voxel_encoder['type'] == 'DynamicScatterVFE'
        self.voxel_layer = Voxelization(**voxel_layer)
        self.voxel_encoder = build_voxel_encoder(voxel_encoder)
        self.timestamp_encoder = TimestampEncoder(timestamp_encoder)
        self.middle_encoder = build_middle_encoder(middle_encoder)
        self.backbone = build_backbone(backbone)
        if segmentation_head is not None:
            self.segmentation_head = build_head(segmentation_head)
            self.segmentation_head.train_cfg, self.segmentation_head.test_cfg = train_cfg, test_cfg
            self.num_classes = segmentation_head['num_classes']
        self.decode_neck = build_neck(decode_neck)
        self.print_info = {}
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.cfg = train_cfg if train_cfg is not None else test_cfg
        self.point_cloud_range, self.voxel_size = voxel_layer['point_cloud_range'], voxel_layer['voxel_size']
        self.voxel_downsampling_size = voxel_downsampling_size
        self.tanh_dims = tanh_dims

    def aug_test(self, *args, **kwargs):
        _refuse('TrackletSegmentor.aug_test')

    @torch.no_grad()
    def voxelize(self, points):
        return self.voxel_layer.voxelize_batch(points)

    def voxel_downsample(self, points_list):
        vs = K.const_tensor(self.voxel_downsampling_size, points_list[0].device)
        lo = K.const_tensor(self.point_cloud_range[:3], points_list[0].device)
        out = []
        for points in points_list:
            coors = torch.div(points[:, :3] - lo[None], vs[None], rounding_mode='floor').long()
            out.append(scatter_v2(points, coors, mode='avg', return_inv=False)[0])
        return out

    def extract_feat(self, points, pts_frame_inds, img_metas=None):
        batch_points, coors = self.voxelize(points)
        pts_frame_inds = torch.cat(pts_frame_inds, 0)
        coors = coors.long()
        pts_with_ts = self.timestamp_encoder(batch_points, pts_frame_inds)
        voxel_features, voxel_coors, voxel2point_inds = self.voxel_encoder(pts_with_ts, coors, return_inv=True)
        voxel_info = self.middle_encoder(voxel_features, voxel_coors)
        if isinstance(voxel_info, dict):
            voxel_info.setdefault('batch_size', len(points))
        x = self.backbone(voxel_info)[0]
        if isinstance(voxel_info, dict) and 'shuffle_inds' in voxel_info:
            raise NotImplementedError('TrackletSegmentor: a voxel-dropping (SST) middle encoder is not built for the tracklet family')
        # the sparse-convolution segmentor drops no voxel: every point is valid, no mask compaction
        out = self.decode_neck(batch_points, coors, x['voxel_feats'], voxel2point_inds, -1, all_valid=True)
        return out, coors, batch_points, pts_frame_inds

    def forward_train(self, points, pts_frame_inds, img_metas=None):
        if self.tanh_dims is not None:
            for p in points:
                p[:, self.tanh_dims] = torch.tanh(p[:, self.tanh_dims])
        elif points[0].size(1) in (4, 5):
            points = [torch.cat([p[:, :3], torch.tanh(p[:, 3:])], dim=1) for p in points]
        if self.voxel_downsampling_size is not None:
            points = self.voxel_downsample(points)
        (feats, _valid), pts_coors, points, pts_frame_inds = self.extract_feat(points, pts_frame_inds, img_metas)
        return dict(seg_points=points, seg_feats=feats, batch_idx=pts_coors[:, 0], pts_frame_inds=pts_frame_inds)

    # the segmentor is a feature extractor: testing is the same pass
    simple_test = forward_train
    forward = forward_train


@DETECTORS.register_module()
class TrackletDetector(nn.Module):
    """detectors/tracklet_detector.py:193-455: the segmentor's point features, then the tracklet RoI head."""

    def __init__(self, segmentor, voxel_layer=None, voxel_encoder=None, middle_encoder=None, neck=None, bbox_head=None, roi_head=None,
                 train_cfg=None, test_cfg=None, pretrained=None, init_cfg=None):
        super().__init__()
        if voxel_layer is not None:
            self.voxel_layer = Voxelization(**voxel_layer)
        if voxel_encoder is not None:
            self.voxel_encoder = build_voxel_encoder(voxel_encoder)
        if middle_encoder is not None:
            self.middle_encoder = build_middle_encoder(middle_encoder)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.cfg = self.train_cfg if self.train_cfg else self.test_cfg
        if _cfg_get(self.cfg, 'pre_voxelization_size', None) is not None:
            _refuse('TrackletDetector: pre_voxelization_size')
        if _cfg_get(test_cfg, 'tta', None) is not None:
            _refuse('TrackletDetector: test_cfg tta')
        self.segmentor = build_detector(segmentor)
        self.num_classes = roi_head['num_classes']
        self.print_info = {}
        roi_head = dict(roi_head)
        roi_head.update(train_cfg=train_cfg, test_cfg=test_cfg)
        roi_head.setdefault('pretrained', pretrained)
        self.roi_head = build_head(roi_head)

    def extract_feat(self):
        pass

    def aug_test(self, *args, **kwargs):
        _refuse('TrackletDetector.aug_test (tta)')

    def _features(self, points, pts_frame_inds, img_metas, tracklet, gt_tracklet_candidates):
        # after PointsRangeFilter there may be an empty input now and then
        points = self.fake_points_for_empty_input(points)
        pts_frame_inds = self.fake_points_for_empty_input(pts_frame_inds)
        self.from_collate_format(tracklet, gt_tracklet_candidates)
        self.tracklet_to_device(tracklet, gt_tracklet_candidates, points[0].device)
        seg = self.segmentor.forward_train(points=points, pts_frame_inds=pts_frame_inds, img_metas=img_metas)
        return dict(pts_xyz=seg['seg_points'][:, :3], pts_feats=seg['seg_feats'], pts_batch_idx=seg['batch_idx'],
                    pts_frame_inds=seg['pts_frame_inds'])

    def forward_train(self, points, pts_frame_inds=None, img_metas=None, tracklet=None, gt_tracklet_candidates=None):
        data = self._features(points, pts_frame_inds, img_metas, tracklet, gt_tracklet_candidates)
        return self.roi_head.forward_train(img_metas=img_metas, tracklet_list=tracklet, gt_candidates_list=gt_tracklet_candidates, **data)

    def simple_test(self, points, img_metas, pts_frame_inds, tracklet, gt_tracklet_candidates=None, rescale=False):
        data = self._features(points, pts_frame_inds, img_metas, tracklet, gt_tracklet_candidates)
        return self.roi_head.simple_test(img_metas=img_metas, tracklet_list=tracklet, gt_candidates_list=gt_tracklet_candidates, **data)

    def forward_test(self, points, img_metas, img=None, **kwargs):
        """batch inference (tracklet_detector.py:425-455): no test-time augmentation"""
        for var, name in [(points, 'points'), (img_metas, 'img_metas')]:
            if not isinstance(var, list):
                raise TypeError('{} must be a list, but got {}'.format(name, type(var)))
        if len(points) != len(img_metas):
            raise ValueError('num of augmentations ({}) != num of image meta ({})'.format(len(points), len(img_metas)))
        return self.simple_test(points, img_metas, **kwargs)

    def forward(self, return_loss=True, **kwargs):
        return self.forward_train(**kwargs) if return_loss else self.forward_test(**kwargs)

    def tracklet_to_device(self, tracklets, candidates_list, device):
        """the predicted tracklets go to the device (one copy each); the candidates stay where they are: the targets pack their
        boxes and timestamps into the step's one host-to-device copy"""
        for t in tracklets:
            t.to(device)

    def from_collate_format(self, tracklets, candidates_list):
        for t in list(tracklets) + [c for cl in (candidates_list or []) for c in cl]:
            if not torch.is_tensor(t.boxes):
                t.from_collate_format()

    def fake_points_for_empty_input(self, points_list):
        return [p.new_zeros((1,) if p.ndim == 1 else (1, p.size(1))) if len(p) == 0 else p for p in points_list]


__all__ = ['TrackletPointRoIExtractor', 'TrackletRoIHead', 'TimestampEncoder', 'TrackletSegmentor', 'TrackletDetector',
           'get_bboxes_from_tracklet', 'LiDARTracklet']
