"""Hot-path mirrors of the detectors that CALL the path (SURVEY.md section 8 "callers either side"): what a config's
``model = dict(type='FSD' | 'SingleStageFSD' | 'FSDV2' | 'SingleStageFSDV2', segmentor=dict(type='VoteSegmentor', ...))``
constructs on the way from points to the features the heads consume, with the reference's constructor arguments,
sub-module names (-> ``state_dict`` keys) and data flow.  Every sub-config whose ``type`` this library implements is BUILT
(Voxelization, DynamicScatterVFE, PseudoMiddleEncoderForSpconvFSD / SSTInputLayerV2, SimpleSparseUNet / SSTv2,
Voxel2PointScatterNeck, VoteSegHead, SIR, ClusterAssigner / SSGAssigner / HybridAssigner, the virtual-voxel stage with multiscale_cfg / as_rpn,
DynamicPointROIExtractor); the rest - box heads, their losses and target assignment, box decoding, NMS - is kept as
its config under ``self.unbuilt`` and never run (the box ops those heads call are in ``sst_amd.box_ops``).  The one loss computed
here is the segmentor's own: VoteSegHead's point targets, decode loss and vote loss (``sst_amd.seg_loss``), which makes
``VoteSegmentor.forward_train`` a whole training step from points and ground-truth boxes to parameter gradients.

Reference:
  VoteSegmentor            mmdet3d/models/detectors/single_stage_fsd.py:155-384 (__init__, voxelize, extract_feat, reorder,
                           forward_train :280-342, the prediction part of simple_test)
  Voxel2PointScatterNeck   mmdet3d/models/necks/voxel2point_neck.py:9-62
  VoteSegHead              mmdet3d/models/decode_heads/segmentation_head.py:16-278 (forward, losses, forward_train,
                           get_targets, decode_vote_targets)
  SingleStageFSD / FSD     single_stage_fsd.py:389-483 (__init__, extract_feat), two_stage_fsd.py (roi_head: config only)
  SingleStageFSDV2 / FSDV2 single_stage_fsd_v2.py:38-271, 375-433 (the stage itself: sst_amd/virtual_voxel.py),
                           two_stage_fsd_v2.py:11-60
  DynamicVoxelNet /        mmdet3d/models/detectors/dynamic_voxelnet.py:10-71, 73-110 (__init__, extract_feat, voxelize): the
  DynamicCenterPoint       detectors of configs/sst_refactor/*.py - the caller of the whole SST hot path
"""
import torch
from torch import nn

from . import fg_group_sample as GS
from . import fg_sample as FS
from . import kernels as K
from . import seg_loss
from ._head_common import cfg_get as _get
from .cluster import ClusterAssigner, HybridAssigner, SSGAssigner
from .registry import BACKBONES, MODELS, ROI_EXTRACTORS, Registry, build_backbone, build_middle_encoder, build_voxel_encoder
from .sst_ops import build_mlp, scatter_v2, unique_with_plan
from .virtual_voxel import VirtualVoxelExtractor
from .voxel import Voxelization

DETECTORS = Registry('detector')
NECKS = Registry('neck')
HEADS = Registry('head')


def build_detector(cfg, train_cfg=None, test_cfg=None):
    """mmdet3d.models.builder.build_detector (builder.py:62-76): train_cfg / test_cfg may come from the outer level"""
    args = dict(cfg)
    if train_cfg is not None:
        args.setdefault('train_cfg', train_cfg)
    if test_cfg is not None:
        args.setdefault('test_cfg', test_cfg)
    return DETECTORS.build(args)


build_model = build_detector


def build_neck(cfg):
    return NECKS.build(cfg)


def build_head(cfg):
    return HEADS.build(cfg)


@NECKS.register_module()
class Voxel2PointScatterNeck(nn.Module):
    """voxel features back onto their points + the point's offset from its voxel centre (necks/voxel2point_neck.py:9-62).

    ``voxel_padding``: rows of dropped voxels (SST-based segmentor with region batching) are filled with it and their points
    masked out; the sparse-convolution segmentor drops nothing, which the caller says with ``all_valid=True``: no mask
    compaction, no host synchronisation."""

    def __init__(self, point_cloud_range=None, voxel_size=None, with_xyz=True, normalize_local_xyz=False):
        super().__init__()
        self.point_cloud_range, self.voxel_size = point_cloud_range, voxel_size
        self.with_xyz, self.normalize_local_xyz = with_xyz, normalize_local_xyz

    def forward(self, points, pts_coors, voxel_feats, voxel2point_inds, voxel_padding=-1, all_valid=False):
        assert points.size(0) == pts_coors.size(0) == voxel2point_inds.size(-1)
        pts_feats = voxel_feats[voxel2point_inds]
        if all_valid:
            pts_mask = torch.ones(points.size(0), dtype=torch.bool, device=points.device)
        else:
            pts_mask = ~((pts_feats == voxel_padding).all(1))
            pts_feats, pts_coors, points = pts_feats[pts_mask], pts_coors[pts_mask], points[pts_mask]
        if not self.with_xyz:
            return pts_feats, pts_mask
        vs = K.const_tensor(self.voxel_size, pts_feats.device, pts_feats.dtype).reshape(1, 3)
        lo = K.const_tensor(self.point_cloud_range[:3], pts_feats.device, pts_feats.dtype).reshape(1, 3)
        center = (pts_coors[:, [3, 2, 1]].to(pts_feats.dtype) + 0.5) * vs + lo
        local_xyz = points[:, :3] - center
        if self.normalize_local_xyz:
            local_xyz = local_xyz / (vs / 2)
        return torch.cat([pts_feats, local_xyz], 1), pts_mask


@HEADS.register_module()
class VoteSegHead(nn.Module):
    """per-point class logits and class-wise centre votes (decode_heads/segmentation_head.py:16-278): the forward pass, the
    vote decoding, and the training side - point targets (points in ground-truth boxes), the decode loss, the vote loss and the
    logged recalls, by the kernels of csrc/seg_loss.hip (``sst_amd.seg_loss``).  Parameters: ``pre_seg_conv`` (build_mlp),
    ``conv_seg``, ``voting`` - the reference's names.

    Built losses: ``loss_decode`` = sigmoid ``FocalLoss`` or softmax ``CrossEntropyLoss`` with mean reduction, ``loss_vote`` =
    ``L1Loss`` with mean reduction.  The configs are parsed at construction without raising (``loss_mode`` says what was found,
    ``loss_unbuilt`` why ``losses`` would refuse); anything else - a ``loss_aux`` among it - raises NotImplementedError when
    ``losses`` is called."""

    def __init__(self, in_channel, num_classes, hidden_dims=(), dropout_ratio=0.5, conv_cfg=dict(type='Conv1d'),
                 norm_cfg=dict(type='naiveSyncBN1d'), act_cfg=dict(type='ReLU'), loss_decode=None, loss_vote=None,
                 loss_aux=None, ignore_index=255, logit_scale=1, checkpointing=False, init_bias=None, init_cfg=None):
        super().__init__()
        hidden_dims = list(hidden_dims)
        end_channel = hidden_dims[-1] if hidden_dims else in_channel
        self.pre_seg_conv = build_mlp(in_channel, hidden_dims, norm_cfg, act=act_cfg['type']) if hidden_dims else None
        self.use_sigmoid = bool((loss_decode or {}).get('use_sigmoid', False))
        self.bg_label = num_classes
        self.num_classes = num_classes if self.use_sigmoid else num_classes + 1       # softmax heads carry a background class
        self.logit_scale = logit_scale
        self.dropout = nn.Dropout(dropout_ratio) if dropout_ratio > 0 else None
        self.conv_seg = nn.Linear(end_channel, self.num_classes)
        self.voting = nn.Linear(end_channel, self.num_classes * 3)
        self.loss_cfg = dict(loss_decode=loss_decode, loss_vote=loss_vote, loss_aux=loss_aux)
        self.train_cfg = self.test_cfg = None
        self.last_counts = None
        self._parse_losses(loss_decode, loss_vote, loss_aux)

    def _parse_losses(self, loss_decode, loss_vote, loss_aux):
        """what ``losses`` will run: never raises (every shipped config constructs), records what it cannot run"""
        # the reference's defaults: CrossEntropyLoss without sigmoid (segmentation_head.py:26-30), L1Loss (:31-33)
        dec = dict(loss_decode) if loss_decode is not None else dict(type='CrossEntropyLoss', use_sigmoid=False)
        vote = dict(loss_vote) if loss_vote is not None else dict(type='L1Loss')
        self.loss_mode, self.loss_unbuilt = None, []
        self.loss_args = dict(gamma=2.0, alpha=0.25, class_weight=None, loss_weight_decode=float(dec.get('loss_weight', 1.0)),
                              loss_weight_vote=float(vote.get('loss_weight', 1.0)))
        plain = dec.get('reduction', 'mean') == 'mean'
        if dec.get('type') == 'FocalLoss' and dec.get('use_sigmoid', True) and plain and \
                isinstance(dec.get('alpha', 0.25), (int, float)):
            self.loss_mode = 'sigmoid_focal'
            self.loss_args.update(gamma=float(dec.get('gamma', 2.0)), alpha=float(dec.get('alpha', 0.25)))
        elif dec.get('type') == 'CrossEntropyLoss' and not dec.get('use_sigmoid', False) and not dec.get('use_mask', False) \
                and plain:
            self.loss_mode = 'softmax_ce'
            self.loss_args.update(class_weight=dec.get('class_weight', None))
        else:
            self.loss_unbuilt.append(f'loss_decode {dec}: only sigmoid FocalLoss and softmax CrossEntropyLoss (mean) are built')
        if not (vote.get('type') == 'L1Loss' and vote.get('reduction', 'mean') == 'mean'):
            self.loss_unbuilt.append(f'loss_vote {vote}: only L1Loss (mean) is built')
        if loss_aux is not None:
            self.loss_unbuilt.append(f'loss_aux {dict(loss_aux)} is not built')

    def forward(self, voxel_feat):
        x = voxel_feat if self.pre_seg_conv is None else self.pre_seg_conv(voxel_feat)
        logits = self.conv_seg(x if self.dropout is None else self.dropout(x))
        return logits, self.voting(x)

    forward_test = forward

    @staticmethod
    def decode_vote_targets(preds):
        return preds * preds.abs()

    @staticmethod
    def encode_vote_targets(delta):
        return torch.sign(delta) * (delta.abs() ** 0.5)

    def get_targets(self, points_list, gt_bboxes_list, gt_labels_list):
        """-> (labels int64 [N], vote_targets [N, 3], vote_mask bool [N]) of the batch (segmentation_head.py:212-275), one
        launch; ``extra_width`` and ``centroid_offset`` come from ``train_cfg``"""
        labels, vote_targets, vote_mask, _ = seg_loss.seg_point_targets(
            points_list, gt_bboxes_list, gt_labels_list, self.bg_label, extra_width=_get(self.train_cfg, 'extra_width', None),
            centroid_offset=bool(_get(self.train_cfg, 'centroid_offset', False)))
        return labels, vote_targets, vote_mask

    def _stat_args(self, device):
        """score thresholds (and, for the softmax head, the group of every class) as cached device vectors"""
        thr = _get(self.train_cfg, 'score_thresh', None)
        if thr is None:
            return None, None, None
        names = list(_get(self.train_cfg, 'class_names'))
        if self.use_sigmoid:
            return K.const_tensor(list(thr), device), None, names[:len(thr)]
        groups = [list(g) for g in _get(self.train_cfg, 'group_names')]
        group_of = [-1] * (self.num_classes - 1)
        for gi, g in enumerate(groups):
            for name in g:
                group_of[names.index(name)] = gi
        return K.const_tensor(list(thr), device), K.const_tensor(group_of, device, torch.int32), names

    def losses(self, seg_logit, vote_preds, seg_label, vote_targets, vote_mask):
        """the reference's dict (segmentation_head.py:106-173): loss_sem_seg, loss_vote, recall_<name> per class and, for the
        softmax head, num_fg.  Three launches and no host read; the reference's asserts on the labels are the status word of
        ``self.last_counts`` (``check_status()``)."""
        if self.loss_unbuilt:
            raise NotImplementedError('; '.join(self.loss_unbuilt))
        thr, group_of, names = self._stat_args(seg_logit.device)
        loss_sem, loss_vote, recall, num_fg, counts = seg_loss.seg_vote_loss(
            seg_logit.float().contiguous(), vote_preds.float().contiguous(), seg_label.contiguous(),
            vote_targets.contiguous(), vote_mask.contiguous(),
            mode=seg_loss.SIGMOID_FOCAL if self.use_sigmoid else seg_loss.SOFTMAX_CE, logit_scale=self.logit_scale,
            score_thresh=thr, class_group=group_of, **self.loss_args)
        self.last_counts = counts
        loss = dict(loss_sem_seg=loss_sem, loss_vote=loss_vote)
        if thr is not None:
            if self.use_sigmoid:
                for i, name in enumerate(names):
                    loss[f'recall_{name}'] = recall[i]
            else:
                for g in _get(self.train_cfg, 'group_names'):
                    for name in g:
                        loss[f'recall_{name}'] = recall[names.index(name)]
                loss['num_fg'] = num_fg
        return loss

    def check_status(self):
        """the reference's asserts on the labels of the last ``losses`` call (segmentation_head.py:124-126, :134-135), for
        whoever wants them: reads one word back"""
        assert self.last_counts is not None, 'no losses() call yet'
        status = int(self.last_counts[1].item())
        assert not status & seg_loss.STATUS_BAD_LABEL, 'a segmentation label lies outside the classes of this head'
        assert not status & seg_loss.STATUS_MASKED_NO_CLASS, 'a point with a vote target carries no class label'

    def forward_train(self, inputs, img_metas, pts_semantic_mask, vote_targets, vote_mask, return_preds=False):
        seg_logits, vote_preds = self.forward(inputs)
        losses = self.losses(seg_logits, vote_preds, pts_semantic_mask, vote_targets, vote_mask)
        if return_preds:
            return losses, dict(seg_logits=seg_logits, vote_preds=vote_preds)
        return losses


@DETECTORS.register_module()
class VoteSegmentor(nn.Module):
    """points -> dynamic voxelisation -> DynamicScatterVFE -> middle encoder -> sparse backbone -> point features -> class
    logits + votes, and in training the head's losses (single_stage_fsd.py:155-384)."""

    def __init__(self, voxel_layer, voxel_encoder, middle_encoder, backbone, segmentation_head, decode_neck=None,
                 auxiliary_head=None, voxel_downsampling_size=None, train_cfg=None, test_cfg=None, init_cfg=None,
                 pretrained=None, tanh_dims=None, **extra_kwargs):
        super().__init__()
        assert voxel_encoder['type'] == 'DynamicScatterVFE'
        self.voxel_layer = Voxelization(**voxel_layer)
        self.voxel_encoder = build_voxel_encoder(voxel_encoder)
        self.middle_encoder = build_middle_encoder(middle_encoder)
        self.backbone = build_backbone(backbone)
        self.segmentation_head = build_head(segmentation_head)
        self.segmentation_head.train_cfg, self.segmentation_head.test_cfg = train_cfg, test_cfg
        self.decode_neck = build_neck(decode_neck)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.cfg = train_cfg if train_cfg is not None else test_cfg
        self.num_classes = segmentation_head['num_classes']
        self.point_cloud_range, self.voxel_size = voxel_layer['point_cloud_range'], voxel_layer['voxel_size']
        self.voxel_downsampling_size = voxel_downsampling_size
        self.tanh_dims = tanh_dims
        self.use_multiscale_features = backbone.get('return_multiscale_features', False)
        self.print_info = {}
        self.unbuilt = {k: v for k, v in dict(auxiliary_head=auxiliary_head).items() if v is not None}
        self._dropped = False

    @torch.no_grad()
    def voxelize(self, points):
        """list of per-sample clouds -> (all points, (b, z, y, x) per point); one launch per sample, no device sync"""
        return self.voxel_layer.voxelize_batch(points)

    def reorder(self, data, shuffle_inds, keep_inds, padding=-1):
        """dropped voxels padded, voxels back in the voxel encoder's order (single_stage_fsd.py:253-266)"""
        temp = data.new_full((len(shuffle_inds), data.size(1)), padding)
        out = data.new_full((len(shuffle_inds), data.size(1)), padding)
        temp[keep_inds] = data
        out[shuffle_inds] = temp
        return out

    def voxel_downsample(self, points_list):
        vs = K.const_tensor(self.voxel_downsampling_size, points_list[0].device)
        lo = K.const_tensor(self.point_cloud_range[:3], points_list[0].device)
        out = []
        for points in points_list:
            coors = torch.div(points[:, :3] - lo[None], vs[None], rounding_mode='floor').long()
            out.append(scatter_v2(points, coors, mode='avg', return_inv=False)[0])
        return out

    def preprocess(self, points):
        """the intensity / elongation squashing and the optional down-sampling both forward_train and simple_test start with
        (single_stage_fsd.py:286-297)"""
        if self.tanh_dims is not None:
            if len(self.tanh_dims) > 0:
                for p in points:
                    p[:, self.tanh_dims] = torch.tanh(p[:, self.tanh_dims])
        elif points[0].size(1) in (4, 5):
            points = [torch.cat([p[:, :3], torch.tanh(p[:, 3:])], dim=1) for p in points]
        if self.voxel_downsampling_size is not None:
            points = self.voxel_downsample(points)
        return points

    def extract_feat(self, points, img_metas=None):
        batch_points, coors = self.voxelize(points)
        coors = coors.long()
        voxel_features, voxel_coors, voxel2point_inds = self.voxel_encoder(batch_points, coors, return_inv=True)
        voxel_info = self.middle_encoder(voxel_features, voxel_coors)
        if isinstance(voxel_info, dict):
            voxel_info.setdefault('batch_size', len(points))
        x = self.backbone(voxel_info)[0]
        padding = -1
        dropped = isinstance(voxel_info, dict) and 'shuffle_inds' in voxel_info
        feats = x['voxel_feats'] if not dropped else \
            self.reorder(x['voxel_feats'], voxel_info['shuffle_inds'], voxel_info['voxel_keep_inds'], padding)
        self._dropped = dropped
        out = self.decode_neck(batch_points, coors, feats, voxel2point_inds, padding, all_valid=not dropped)
        if self.use_multiscale_features:
            return out, coors, batch_points, x['decoder_features']
        return out, coors, batch_points

    def forward(self, points, img_metas=None):
        """the prediction half of simple_test / forward_train(as_subsegmentor=True): -> dict(seg_points, seg_logits,
        seg_vote_preds, offsets, seg_feats, batch_idx, decoder_features)"""
        points = self.preprocess(points)
        res = self.extract_feat(points, img_metas)
        (feats, valid), pts_coors, batch_points = res[0], res[1], res[2]
        decoder_features = res[3] if self.use_multiscale_features else None
        if self._dropped:           # SST-based segmentor: points of dropped voxels leave; the sparse-convolution one keeps all
            batch_points, pts_coors = batch_points[valid], pts_coors[valid]
        seg_logits, vote_preds = self.segmentation_head(feats)
        return dict(seg_points=batch_points, seg_logits=seg_logits, seg_vote_preds=vote_preds,
                    offsets=self.segmentation_head.decode_vote_targets(vote_preds), seg_feats=feats,
                    batch_idx=pts_coors[:, 0], decoder_features=decoder_features)

    simple_test = forward

    def forward_train(self, points, img_metas, gt_bboxes_3d, gt_labels_3d, as_subsegmentor=False):
        """points + ground-truth boxes -> the loss dict (single_stage_fsd.py:280-342); with ``as_subsegmentor`` the output dict
        of ``forward`` plus ``losses`` - what the FSD detectors run in every training step"""
        points = self.preprocess(points)
        labels, vote_targets, vote_mask = self.segmentation_head.get_targets(points, gt_bboxes_3d, gt_labels_3d)
        res = self.extract_feat(points, img_metas)
        (feats, valid), pts_coors, batch_points = res[0], res[1], res[2]
        decoder_features = res[3] if self.use_multiscale_features else None
        if self._dropped:           # only the SST-based segmentor drops voxels: no compaction otherwise
            batch_points, pts_coors = batch_points[valid], pts_coors[valid]
            labels, vote_targets, vote_mask = labels[valid], vote_targets[valid], vote_mask[valid]
        assert feats.size(0) == labels.size(0)
        losses, preds = self.segmentation_head.forward_train(feats, img_metas, labels, vote_targets, vote_mask,
                                                             return_preds=True)
        if not as_subsegmentor:
            return losses
        return dict(seg_points=batch_points, seg_logits=preds['seg_logits'], seg_vote_preds=preds['vote_preds'],
                    offsets=self.segmentation_head.decode_vote_targets(preds['vote_preds']), seg_feats=feats,
                    batch_idx=pts_coors[:, 0], losses=losses, decoder_features=decoder_features)


@DETECTORS.register_module()
class DynamicVoxelNet(nn.Module):
    """points -> dynamic voxelisation -> DynamicVFE -> SSTInputLayerV2 -> SSTv2 (dynamic_voxelnet.py:10-71): what
    ``model = dict(type='DynamicVoxelNet', voxel_layer=..., voxel_encoder=..., middle_encoder=..., backbone=..., neck=...,
    bbox_head=...)`` of configs/sst_refactor/*.py constructs up to the backbone's output, with the reference's constructor
    arguments and sub-module names (-> ``state_dict`` keys ``voxel_encoder.*``, ``backbone.*``).  The dense BEV neck (SECOND
    FPN) and the box head are opt-in: their configs are kept under ``self.unbuilt`` until ``attach_heads()`` builds them as
    ``neck`` / ``bbox_head``; then ``forward_train`` and ``simple_test`` follow the reference (VoxelNet's), before that they
    raise.

    ``extract_feat`` has the reference's semantics (:38-47: voxelize -> voxel_encoder -> middle_encoder(.., batch_size) ->
    backbone).  When the three index stages are the ones the fused frame plan covers (csrc/frame_plan.hip: DynamicVFE +
    SSTInputLayerV2 on the same grid, voxels allowed to leave in window-major order - automatic with ``shuffle_voxels=True``)
    the same results come from ONE device-side plan per batch: no host round trip until the voxel encoder's kernels are
    queued (the reference reads ``coors[-1, 0].item()`` and three sizes back; the piecewise path of this package one size per
    module boundary).  ``fused_index = False`` forces the piecewise path; ``prepare()`` builds the plan of a batch ahead of
    time (it depends on the point clouds only - what a data-loader prefetch would do) for ``extract_feat(.., prepared=)``."""

    def __init__(self, voxel_layer, voxel_encoder, middle_encoder, backbone, neck=None, bbox_head=None, train_cfg=None,
                 test_cfg=None, pretrained=None, init_cfg=None):
        super().__init__()
        self.voxel_layer = Voxelization(**voxel_layer)
        self.voxel_encoder = build_voxel_encoder(voxel_encoder)
        self.middle_encoder = build_middle_encoder(middle_encoder)
        self.backbone = build_backbone(backbone)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.unbuilt = {k: v for k, v in dict(neck=neck, bbox_head=bbox_head).items() if v is not None}
        self.fused_index = True
        self._planner = None

    with_neck = False          # until attach_heads() builds the dense neck, extract_feat ends at the backbone's output

    @torch.no_grad()
    def voxelize(self, points):
        """list of per-sample clouds -> (all points, (b, z, y, x) int32 per point) (dynamic_voxelnet.py:49-71)"""
        return self.voxel_layer.voxelize_batch(points)

    def _frame_planner(self, batch_size):
        # (written against `self` = ANY detector object with voxel_layer / voxel_encoder / middle_encoder sub-modules: the
        # reference's own DynamicVoxelNet instance after install_fused_extract_feat(), whose class never set these attributes)
        from .frame_plan import FramePlanner
        from .sst_input_layer import SSTInputLayerV2
        from .voxel_encoder import DynamicVFE
        if not getattr(self, 'fused_index', True):
            return None
        planner = self.__dict__.get('_planner')
        if planner is None:
            ok = (type(self.voxel_encoder) is DynamicVFE and type(self.middle_encoder) is SSTInputLayerV2
                  and isinstance(self.voxel_layer, Voxelization) and hasattr(self.voxel_encoder, '_grid_zyx'))
            planner = FramePlanner(self.voxel_layer, self.voxel_encoder, self.middle_encoder) if ok else False
            self.__dict__['_planner'] = planner
        return planner if (planner and planner.supported(batch_size)) else None

    def prepare(self, points, overlap=False, ready_event=None):
        """the index work of one batch (voxelize, point -> voxel grouping, window bucketing / drop / window CSR, positional
        rows): a FramePlan, or None when the fused plan does not cover this configuration / batch (extract_feat then runs the
        piecewise path itself).

        ``overlap=True`` (a data-loader hook's mode): the plan is built on a stream of its own, concurrently with the step the
        caller's stream is still working on; the point clouds must be complete, or complete once ``ready_event`` has happened
        (FramePlanner.build_overlapped).  Host tensors (the data loader's pinned batch) are copied to the device on that
        stream first - then nothing has to be promised."""
        if len(points) == 0:
            return None
        planner = DynamicVoxelNet._frame_planner(self, len(points))
        if planner is None:
            return None
        if overlap and not any(p.is_cuda for p in points):
            return planner.build_overlapped_from_host(points, next(self.parameters()).device)
        if not all(p.is_cuda for p in points):
            return None
        return planner.build_overlapped(points, ready_event) if overlap else planner.build(points)

    def voxel_info(self, points, prepared=None):
        """everything in front of the backbone: -> the ``voxel_info`` dictionary SSTInputLayerV2 returns"""
        plan = prepared if prepared is not None else DynamicVoxelNet.prepare(self, points)
        if plan is not None:     # the voxel encoder is queued before the plan's sizes are read (FramePlan.finalize)
            voxel_features, _ = self.voxel_encoder(plan.points, plan.coors, scatter_plan=plan)
            return plan.finalize(voxel_features, self.middle_encoder)
        voxels, coors = self.voxelize(points)          # the detector's own voxelize(): the reference's per-sample loop works too
        voxel_features, feature_coors = self.voxel_encoder(voxels, coors)
        return self.middle_encoder(voxel_features, feature_coors, len(points))

    def extract_feat(self, points, img_metas=None, prepared=None):
        x = self.backbone(self.voxel_info(points, prepared))
        if self.with_neck:
            x = self.neck(x)
        return x

    def extract_voxel_feats(self, points, img_metas=None, prepared=None):
        """the path up to the shift blocks' output, whatever the backbone's ``to_bev`` says: (features [M', C] of the kept
        voxels, their (b, z, y, x)) - the part of ``extract_feat`` SURVEY.md section 8(d) defines the frames/s metric on"""
        info = self.voxel_info(points, prepared)
        return self.backbone.forward_voxels(info), info['voxel_coors']

    forward = extract_feat

    def attach_heads(self):
        """Opt in to the training and test steps: build the neck and the box head whose configs are parked in ``self.unbuilt``
        (``build_neck(unbuilt['neck'])``, ``build_head(dict(unbuilt['bbox_head'], train_cfg=.., test_cfg=..))`` followed by the
        head's ``attach_network()`` where it has one) and let ``extract_feat`` end at the neck, as dynamic_voxelnet.py:38-47
        does.  ``unbuilt`` stays as it is; a detector without this call constructs and behaves exactly as before.  Written
        against ``self`` = any detector object with ``unbuilt`` / ``train_cfg`` / ``test_cfg``.  -> self"""
        if 'bbox_head' not in self.unbuilt:
            raise RuntimeError(f'{type(self).__name__}.attach_heads: the config has no bbox_head')
        if 'neck' in self.unbuilt:
            self.neck = build_neck(self.unbuilt['neck'])
            self.with_neck = True
        head = build_head(dict(self.unbuilt['bbox_head'], train_cfg=self.train_cfg, test_cfg=self.test_cfg))
        if hasattr(head, 'attach_network'):
            head.attach_network()
        self.bbox_head = head
        return self

    def _require_heads(self, what):
        if getattr(self, 'bbox_head', None) is None:
            raise NotImplementedError(f'{type(self).__name__}.{what}: the box head, its losses and target assignment are not built '
                                      '- call attach_heads() first (the detector parks the neck\'s and the head\'s configs in '
                                      '`unbuilt` until then)')

    def forward_train(self, points, img_metas, gt_bboxes_3d, gt_labels_3d, gt_bboxes_ignore=None):
        """VoxelNet.forward_train (detectors/voxelnet.py): bbox_head.loss(*outs, gt_bboxes_3d, gt_labels_3d, img_metas, ..)"""
        self._require_heads('forward_train')
        x = self.extract_feat(points, img_metas)
        outs = self.bbox_head(x)
        return self.bbox_head.loss(*outs, gt_bboxes_3d, gt_labels_3d, img_metas, gt_bboxes_ignore=gt_bboxes_ignore)

    def simple_test(self, points, img_metas, imgs=None, rescale=False):
        """VoxelNet.simple_test: bbox_head.get_bboxes(*outs, img_metas) -> bbox3d2result per sample"""
        self._require_heads('simple_test')
        x = self.extract_feat(points, img_metas)
        outs = self.bbox_head(x)
        bbox_list = self.bbox_head.get_bboxes(*outs, img_metas, rescale=rescale)
        return [bbox3d2result(bboxes, scores, labels) for bboxes, scores, labels in bbox_list]

    def aug_test(self, *args, **kwargs):
        raise NotImplementedError(f'{type(self).__name__}.aug_test: test-time augmentation is not built')

    def losses(self, *args, **kwargs):
        raise NotImplementedError('the box head, its losses and target assignment are outside the hot path (SURVEY.md section 8)')


@DETECTORS.register_module()
class DynamicCenterPoint(DynamicVoxelNet):
    """dynamic_voxelnet.py:73-136: the same feature path with CenterHead on top; the steps after ``attach_heads()``"""

    def forward_train(self, points, img_metas, gt_bboxes_3d, gt_labels_3d, gt_bboxes_ignore=None):
        self._require_heads('forward_train')
        x = self.extract_feat(points, img_metas)
        outs = self.bbox_head(x)
        return self.bbox_head.loss(gt_bboxes_3d, gt_labels_3d, outs)

    def simple_test(self, points, img_metas, imgs=None, rescale=False):
        self._require_heads('simple_test')
        x = self.extract_feat(points, img_metas)
        outs = self.bbox_head(x)
        bbox_list = self.bbox_head.get_bboxes(outs, img_metas, rescale=rescale)
        return [bbox3d2result(bboxes, scores, labels) for bboxes, scores, labels in bbox_list]


def install_fused_extract_feat(detector_cls):
    """Reference-side hook: give the REFERENCE's own detector class - mmdet3d's DynamicVoxelNet /
    DynamicCenterPoint, which keeps its neck, heads, losses and test-time code - the ``extract_feat`` of this module: same
    semantics as detectors/dynamic_voxelnet.py:38-47 (voxelize -> voxel_encoder -> middle_encoder(.., batch_size) -> backbone
    -> neck), with the three index stages as ONE device-side plan when the sub-modules are this library's.

        from mmdet3d.models.detectors import DynamicVoxelNet, DynamicCenterPoint
        sst_amd.detectors.install_fused_extract_feat(DynamicVoxelNet)        # DynamicCenterPoint inherits it
    """
    def extract_feat(self, points, img_metas=None):
        x = self.backbone(DynamicVoxelNet.voxel_info(self, points))
        if getattr(self, 'with_neck', False):
            x = self.neck(x)
        return x

    extract_feat.__doc__ = 'Extract features from points (sst_amd: fused index plan in front of the backbone).'
    detector_cls.extract_feat = extract_feat
    return detector_cls


def bbox3d2result(bboxes, scores, labels):
    """mmdet3d.core.bbox3d2result: the results of one sample on the host"""
    return dict(boxes_3d=bboxes.to('cpu'), scores_3d=scores.cpu(), labels_3d=labels.cpu())


class _HotPathDetector(nn.Module):
    """shared: the segmentor, the record of what was not built"""

    def _init_common(self, segmentor, bbox_head, train_cfg, test_cfg, **others):
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.cfg = train_cfg if train_cfg else test_cfg
        self.segmentor = build_detector(segmentor)
        self.head_type = bbox_head['type']
        self.num_classes = bbox_head['num_classes']
        self.as_rpn = bool(bbox_head.get('as_rpn', False))
        self.unbuilt = {'bbox_head': bbox_head}
        self.unbuilt.update({k: v for k, v in others.items() if v is not None})
        self.print_info, self.runtime_info = {}, {}

    def combine_classes(self, data_dict, name_list):
        """single_stage_fsd.py:588-593.  A dictionary that ``update_sample_results_by_mask`` made over the kernels carries the
        classes combined already (``data_dict['combined']``: one gather wrote them); any other dictionary of per-class lists is
        concatenated as the reference does."""
        done = data_dict.get('combined') if isinstance(data_dict, dict) else None
        if done is not None:
            return {name: done[name] for name in name_list if name in done}
        return {name: torch.cat(data_dict[name], 0) for name in data_dict if name in name_list}

    def attach_heads(self):
        """Opt in to the training and test steps: build the heads whose configs are parked in ``self.unbuilt`` as submodules, by
        the calls the heads document (``build_head(dict(det.unbuilt['bbox_head'], train_cfg=det.train_cfg,
        test_cfg=det.test_cfg))``; ``roi_head`` with the ``rcnn`` parts).  ``unbuilt`` stays as it is; a detector without this
        call constructs exactly as before (same ``state_dict`` keys).  -> self"""
        cfg = self.unbuilt['bbox_head']
        if cfg.get('type') != 'SparseClusterHeadV2':
            raise NotImplementedError(f"attach_heads: bbox_head {cfg.get('type')} - the FSD step is built over SparseClusterHeadV2 "
                                      '(FSDV2Head / SingleStageFSDV2 / FSDV2 are out of scope)')
        self.bbox_head = build_head(dict(cfg, train_cfg=self.train_cfg, test_cfg=self.test_cfg))
        roi = self.unbuilt.get('roi_head')
        if roi is not None:
            self.roi_head = build_head(dict(roi, train_cfg=_get(self.train_cfg, 'rcnn', None), test_cfg=_get(self.test_cfg, 'rcnn', None)))
        return self

    def _require_heads(self, what):
        if getattr(self, 'bbox_head', None) is None or ('roi_head' in self.unbuilt and getattr(self, 'roi_head', None) is None):
            raise RuntimeError(f'{type(self).__name__}.{what}: the heads are not built - call attach_heads() first (the detector '
                               'parks their configs in `unbuilt` until then)')


@DETECTORS.register_module()
class SingleStageFSD(_HotPathDetector):
    """segmentor -> (sampling, clustering: ``cluster_assigner``) -> SIR backbone over the clusters
    (single_stage_fsd.py:389-483)."""

    def __init__(self, backbone, segmentor, voxel_layer=None, voxel_encoder=None, middle_encoder=None, neck=None,
                 bbox_head=None, train_cfg=None, test_cfg=None, cluster_assigner=None, pretrained=None, init_cfg=None):
        super().__init__()
        self._init_common(segmentor, bbox_head, train_cfg, test_cfg, neck=neck)
        self.backbone = build_backbone(backbone)
        if voxel_layer is not None:
            self.voxel_layer = Voxelization(**voxel_layer)
        if voxel_encoder is not None:
            self.voxel_encoder = build_voxel_encoder(voxel_encoder)
        if middle_encoder is not None:
            self.middle_encoder = build_middle_encoder(middle_encoder)
        if 'radius' in cluster_assigner:                                     # single_stage_fsd.py:429-435
            self.cluster_assigner = SSGAssigner(**cluster_assigner)
        elif 'hybrid' in cluster_assigner:
            cluster_assigner.pop('hybrid')
            self.cluster_assigner = HybridAssigner(**cluster_assigner)
        else:
            self.cluster_assigner = ClusterAssigner(**cluster_assigner)
        self.cluster_assigner.num_classes = self.num_classes

    def extract_feat(self, points, pts_feats, pts_cluster_inds, img_metas, center_preds):
        cluster_xyz, _, inv_inds = scatter_v2(center_preds, pts_cluster_inds, mode='avg', return_inv=True)
        f_cluster = points[:, :3] - cluster_xyz[inv_inds]
        out_pts_feats, cluster_feats, out_coors = self.backbone(points, pts_feats, pts_cluster_inds, f_cluster)
        out = dict(cluster_feats=cluster_feats, cluster_xyz=cluster_xyz, cluster_inds=out_coors)
        if self.as_rpn:
            out['cluster_pts_feats'], out['cluster_pts_xyz'] = out_pts_feats, points
        return out

    # ------------------------------------------------------------------------------------------------------------------
    # the stage between the segmentor and the clustering (single_stage_fsd.py:571-615, 698-816) over csrc/fg_sample.hip
    # ------------------------------------------------------------------------------------------------------------------
    def pre_voxelize(self, data_dict):
        """single_stage_fsd.py:595-615: one grouping (``unique_with_plan``), one segmented mean per float tensor over its plan"""
        batch_idx, points = data_dict['batch_idx'], data_dict['seg_points']
        vs = K.const_tensor(self.cfg['pre_voxelization_size'], points.device)
        lo = K.const_tensor(self.cluster_assigner.point_cloud_range[:3], points.device)
        coors = torch.div(points[:, :3] - lo[None], vs[None], rounding_mode='floor').long()[:, [2, 1, 0]]
        coors = torch.cat([batch_idx.long()[:, None], coors], dim=1)
        new_coors, unq_inv = unique_with_plan(coors)
        out = {}
        for name, data in data_dict.items():
            if torch.is_tensor(data) and data.dtype in (torch.float, torch.float16):
                out[name] = scatter_v2(data, coors, mode='avg', return_inv=False, new_coors=new_coors, unq_inv=unq_inv)[0]
        out['batch_idx'] = new_coors[:, 0]
        return out

    def _fg_inputs(self, seg_logits, seg_points, batch_idx, gt_bboxes_3d, gt_labels_3d):
        """what get_fg_mask decides per class (:756-797) as the kernel's inputs: (float32-rounded thresholds, extra mask)"""
        cfg = self.train_cfg if self.training else self.test_cfg
        n_cls, extra = self.num_classes, None
        if self.training and _get(self.train_cfg, 'disable_pretrain', False) and not self.runtime_info.get('enable_detection', False):
            topks = _get(self.train_cfg, 'disable_pretrain_topks', [100, 100, 100])
            thr = [float('inf')] * n_cls                 # the top-k indices replace the threshold
            extra = FS.topk_extra_mask(seg_logits, topks)
        else:
            buffer_thr = self.runtime_info.get('threshold_buffer', 0) if (self.training and self.runtime_info is not None) else 0
            thr = FS.round_thresholds(list(self.cfg['score_thresh'])[:n_cls], buffer_thr)
        if _get(cfg, 'add_gt_fg_points', False):
            extra = FS.gt_extra_mask(seg_points, batch_idx, gt_bboxes_3d, gt_labels_3d, n_cls, out=extra)
        return thr, extra

    def _num_samples(self, batch_idx, batch_size=None):
        if batch_size is None:
            batch_size = getattr(self, '_batch_size', None)
        if batch_size is None:                           # called outside forward_train / simple_test: one read, as the reference
            batch_size = int(batch_idx[-1].item()) + 1 if batch_idx.numel() else 1
        return batch_size

    def get_fg_mask(self, seg_scores, seg_points, cls_id, batch_inds, gt_bboxes_3d, gt_labels_3d, seg_logits=None):
        """single_stage_fsd.py:756-797 for one class, over the sampling kernel (without the at-least-one-point rule, as there).
        The kernel thresholds the library's own sigmoid of the LOGITS: pass them as ``seg_logits`` (``seg_scores`` is not
        read)."""
        if seg_logits is None:
            raise NotImplementedError('get_fg_mask: pass seg_logits= (the kernel decides on the logits; scores alone are not enough)')
        thr, extra = self._fg_inputs(seg_logits, seg_points, batch_inds, gt_bboxes_3d, gt_labels_3d)
        pend = FS.fg_sample_launch(seg_logits, None, seg_points, batch_inds, thr, self._num_samples(batch_inds), extra,
                                   apply_rule=False)
        return pend.mask[cls_id]

    def sample(self, dict_to_sample, offset, gt_bboxes_3d=None, gt_labels_3d=None, batch_size=None):
        """single_stage_fsd.py:698-748 over ``fg_sample``: the reference's per-class lists ``seg_points``, ``batch_idx``,
        ``center_preds``, ``fg_mask_list`` (+ ``src``, ``slot``, ``class_offsets``, ``totals``, ``rule``).  The wide tensors
        (``seg_logits``, ``seg_vote_preds``, ``seg_feats``) are NOT copied per class here: ``update_sample_results_by_mask``
        gathers them once, after the cluster filter, from ``source`` (the input dictionary, which rides along).  One host read.
        The reference's ``assert (seg_logits < 0).any()`` - a device read for a debugging check - is dropped."""
        if _get(self.cfg, 'group_sample', False):
            return self.group_sample(dict_to_sample, offset, gt_bboxes_3d, gt_labels_3d, batch_size)
        seg_logits = dict_to_sample['seg_logits']
        if seg_logits.size(1) != self.num_classes:
            raise NotImplementedError('SingleStageFSD.sample: seg_logits with a background column (the softmax score path, '
                                      'group_sample) is not built')
        seg_points, batch_idx = dict_to_sample['seg_points'], dict_to_sample['batch_idx']
        thr, extra = self._fg_inputs(seg_logits, seg_points, batch_idx, gt_bboxes_3d, gt_labels_3d)
        out = dict(FS.fg_sample(seg_logits, offset, seg_points, batch_idx, thr, self._num_samples(batch_idx, batch_size), extra))
        out['source'] = dict_to_sample
        return out

    # the softmax score path (single_stage_fsd.py:818-919) over csrc/fg_group_sample.hip: a "class" downstream is a GROUP
    def _groups(self):
        """the groups of ``cfg.group_names`` as lists of class indices, after the refusals by name"""
        cfg = self.train_cfg if self.training else self.test_cfg
        if _get(self.cfg, 'offset_weight', 'max') != 'max':
            raise NotImplementedError(f"SingleStageFSD.get_offset_weight: offset_weight {self.cfg['offset_weight']!r} (only 'max', "
                                      'as in the reference)')
        if _get(cfg, 'add_gt_fg_points', False):
            raise NotImplementedError('SingleStageFSD.group_sample: add_gt_fg_points with group_sample (the reference passes no '
                                      'boxes to get_fg_mask there and cannot run it)')
        if _get(self.cfg, 'group_names', None) is None or _get(self.cfg, 'class_names', None) is None:
            raise NotImplementedError('SingleStageFSD.group_sample: the config sets group_sample without group_names / class_names')
        groups = GS.groups_by_names(self.cfg['group_names'], self.cfg['class_names'])
        if len(groups) != len(self.cfg['score_thresh']):
            raise RuntimeError(f"SingleStageFSD.group_sample: {len(groups)} groups for {len(self.cfg['score_thresh'])} score thresholds")
        return GS.check_groups(groups, self.num_classes + 1)

    def group_sample(self, dict_to_sample, offset, gt_bboxes_3d=None, gt_labels_3d=None, batch_size=None):
        """single_stage_fsd.py:818-881 over ``fg_group_sample.group_sample``: fp32 softmax over ``num_classes + 1`` logits, the
        scores summed per group (background excluded), ``score_thresh`` per group (+ ``threshold_buffer``), the at-least-one-point
        rule per (group, sample), the centre ``point + sum_k w_k offset_k`` with the ``'max'`` weights.  -> per-GROUP lists in the
        layout of ``sample``; ``disable_pretrain`` takes ``disable_pretrain_topks`` with one entry per group.  One host read."""
        seg_logits = dict_to_sample['seg_logits']
        groups = self._groups()
        if seg_logits.size(1) != self.num_classes + 1:
            raise NotImplementedError(f'SingleStageFSD.group_sample: seg_logits must have num_classes + 1 = {self.num_classes + 1} '
                                      f'columns (the background last), got {seg_logits.size(1)}')
        seg_points, batch_idx = dict_to_sample['seg_points'], dict_to_sample['batch_idx']
        if self.training and _get(self.train_cfg, 'disable_pretrain', False) and not self.runtime_info.get('enable_detection', False):
            topks = list(_get(self.train_cfg, 'disable_pretrain_topks', [100, 100, 100]))
            if len(topks) != len(groups):
                raise NotImplementedError(f'SingleStageFSD.group_sample: disable_pretrain_topks has {len(topks)} entries for '
                                          f'{len(groups)} groups')
            thr, extra = [float('inf')] * len(groups), GS.group_topk_extra_mask(seg_logits, groups, topks)
        else:
            buffer_thr = self.runtime_info.get('threshold_buffer', 0) if (self.training and self.runtime_info is not None) else 0
            thr, extra = FS.round_thresholds(list(self.cfg['score_thresh']), buffer_thr), None
        out = dict(GS.group_sample(seg_logits, offset, seg_points, batch_idx, groups, thr, self._num_samples(batch_idx, batch_size),
                                   1, extra))
        out['source'] = dict_to_sample
        return out

    def gather_group_by_names(self, scores):
        """single_stage_fsd.py:907-919: [N, num_classes] scores -> [N, G], the columns of every group summed"""
        groups = GS.groups_by_names(self.cfg['group_names'], self.cfg['class_names'])
        return torch.stack([scores[:, g].sum(1) for g in groups], dim=1)

    def gather_group(self, scores, group_lens):
        """single_stage_fsd.py:893-905: consecutive column runs of the given lengths summed"""
        assert sum(group_lens) == scores.size(1)
        return torch.stack([s.sum(1) for s in torch.split(scores, list(group_lens), dim=1)], dim=1)

    def get_offset_weight(self, seg_logit):
        """single_stage_fsd.py:883-891: 1 on the maxima of a row (within 1e-6), shared among equal maxima"""
        if _get(self.cfg, 'offset_weight', 'max') != 'max':
            raise NotImplementedError(f"SingleStageFSD.get_offset_weight: offset_weight {self.cfg['offset_weight']!r} (only 'max', "
                                      'as in the reference)')
        weight = ((seg_logit - seg_logit.max(1)[0][:, None]).abs() < 1e-6).float()
        return weight / weight.sum(1)[:, None]

    def update_sample_results_by_mask(self, sampled_out, valid_mask_list):
        """single_stage_fsd.py:571-586 over ``fg_gather_cat``: the narrow per-class lists are indexed by the assigner's
        ``valid_mask`` (its ``_sst_keep`` index list: no search), the final masks come from one small launch, and the wide rows
        of all classes are gathered ONCE into ``combined`` (``pts_feats`` = logits | vote predictions | features, ``seg_points``,
        ``center_preds``), which ``combine_classes`` hands out.  The reference's ``assert new_data.sum() == mask.sum()`` (a
        device read) is dropped."""
        src = sampled_out['source']
        detach = bool(_get(self.train_cfg, 'detach_segmentor', False)) if self.training else False
        out = FS.fg_gather_cat(sampled_out, valid_mask_list, src['seg_logits'], src['seg_vote_preds'], src['seg_feats'],
                               src['seg_points'], detach_feats=detach)
        keeps = [FS.keep_of(v) if v.dtype == torch.bool else v for v in valid_mask_list]
        new = dict(sampled_out)
        for name in ('seg_points', 'batch_idx', 'center_preds'):
            new[name] = [d[k] for d, k in zip(sampled_out[name], keeps)]
        n_l, n_v = src['seg_logits'].size(1), src['seg_vote_preds'].size(1)
        feats = out['pts_feats']
        new['fg_mask_list'] = out['fg_mask_list']
        new['slot2'] = out['slot2']
        new['combined'] = dict(seg_points=out['seg_points'], center_preds=out['center_preds'], pts_feats=feats,
                               seg_logits=feats[:, :n_l], seg_vote_preds=feats[:, n_l:n_l + n_v], seg_feats=feats[:, n_l + n_v:])
        return new

    def _cluster_step(self, seg_out_dict, seg_feats, img_metas, gt_bboxes_3d, gt_labels_3d, train):
        """what forward_train (:508-543) and simple_test (:636-667) share between the segmentor and the box head"""
        det = (lambda t: t.detach()) if train else (lambda t: t)
        dict_to_sample = dict(seg_points=seg_out_dict['seg_points'], seg_logits=det(seg_out_dict['seg_logits']),
                              seg_vote_preds=det(seg_out_dict['seg_vote_preds']), seg_feats=seg_feats,
                              batch_idx=seg_out_dict['batch_idx'], vote_offsets=det(seg_out_dict['offsets']))
        if _get(self.cfg, 'pre_voxelization_size', None) is not None:
            dict_to_sample = self.pre_voxelize(dict_to_sample)
        sampled_out = self.sample(dict_to_sample, dict_to_sample['vote_offsets'], gt_bboxes_3d, gt_labels_3d)
        cluster_inds_list, valid_mask_list = self.cluster_assigner(sampled_out['center_preds'], sampled_out['batch_idx'],
                                                                   gt_bboxes_3d, gt_labels_3d,
                                                                   origin_points=sampled_out['seg_points'])
        pts_cluster_inds = torch.cat(cluster_inds_list, dim=0)            # (class, sample, cluster) per point
        sampled_out = self.update_sample_results_by_mask(sampled_out, valid_mask_list)
        combined_out = self.combine_classes(sampled_out, ['seg_points', 'pts_feats', 'center_preds'])
        points, pts_feats = combined_out['seg_points'], combined_out['pts_feats']
        assert len(pts_cluster_inds) == len(points) == len(pts_feats)
        extracted_outs = self.extract_feat(points, pts_feats, pts_cluster_inds, img_metas, combined_out['center_preds'])
        outs = self.bbox_head(extracted_outs['cluster_feats'], extracted_outs['cluster_xyz'], extracted_outs['cluster_inds'])
        return dict_to_sample, sampled_out, points, extracted_outs, outs

    def forward_train(self, points, img_metas, gt_bboxes_3d, gt_labels_3d, gt_bboxes_ignore=None, runtime_info=None):
        """single_stage_fsd.py:487-569: points and ground-truth boxes -> the loss dictionary (segmentor losses, num_clusters,
        num_fg_points, the cluster head's losses), or with ``as_rpn`` the reference's output dictionary for the RoI stage.
        ``num_clusters`` is the row count of the grouping ``extract_feat`` makes anyway, not a further ``unique``; the
        reference's asserts that read the device (``(seg_logits < 0).any()``, ``cluster_inds[:, 0].max().item()``) are dropped."""
        self._require_heads('forward_train')
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
        dict_to_sample, sampled_out, fg_points, extracted_outs, outs = self._cluster_step(
            seg_out_dict, seg_feats, img_metas, gt_bboxes_3d, gt_labels_3d, train=True)
        cluster_xyz, cluster_inds = extracted_outs['cluster_xyz'], extracted_outs['cluster_inds']
        dev = fg_points.device
        losses['num_clusters'] = torch.ones((1,), device=dev).float() * cluster_xyz.size(0)
        losses['num_fg_points'] = torch.ones((1,), device=dev).float() * len(fg_points)
        det_loss = self.bbox_head.loss(outs['cls_logits'], outs['reg_preds'], cluster_xyz, cluster_inds, gt_bboxes_3d,
                                       gt_labels_3d, img_metas, iou_logits=outs.get('iou_logits', None),
                                       gt_bboxes_ignore=gt_bboxes_ignore)
        if hasattr(self.bbox_head, 'print_info'):
            self.print_info.update(self.bbox_head.print_info)
        losses.update(det_loss)
        losses.update(self.print_info)
        if not self.as_rpn:
            return losses
        return dict(rpn_losses=losses, cls_logits=outs['cls_logits'], reg_preds=outs['reg_preds'], cluster_xyz=cluster_xyz,
                    cluster_inds=cluster_inds, all_input_points=dict_to_sample['seg_points'],
                    valid_pts_feats=extracted_outs['cluster_pts_feats'], valid_pts_xyz=extracted_outs['cluster_pts_xyz'],
                    seg_feats=dict_to_sample['seg_feats'], pts_mask=sampled_out['fg_mask_list'],
                    pts_batch_inds=dict_to_sample['batch_idx'])

    def simple_test(self, points, img_metas, imgs=None, rescale=False, gt_bboxes_3d=None, gt_labels_3d=None):
        """single_stage_fsd.py:621-691 (one sample); the reference's ``assert (cluster_inds[:, 1] == 0).all()`` (a device read)
        is dropped"""
        self._require_heads('simple_test')
        if gt_bboxes_3d is not None:
            gt_bboxes_3d, gt_labels_3d = gt_bboxes_3d[0], gt_labels_3d[0]
            assert isinstance(gt_bboxes_3d, list) and isinstance(gt_labels_3d, list)
            assert len(gt_bboxes_3d) == len(gt_labels_3d) == 1, 'assuming single sample testing'
            gt_bboxes_3d = [b[l >= 0] for b, l in zip(gt_bboxes_3d, gt_labels_3d)]
            gt_labels_3d = [l[l >= 0] for l in gt_labels_3d]
        self._batch_size = len(points)
        seg_out_dict = self.segmentor.simple_test(points, img_metas)
        dict_to_sample, sampled_out, _, extracted_outs, outs = self._cluster_step(
            seg_out_dict, seg_out_dict['seg_feats'], img_metas, gt_bboxes_3d, gt_labels_3d, train=False)
        bbox_list = self.bbox_head.get_bboxes(outs['cls_logits'], outs['reg_preds'], extracted_outs['cluster_xyz'],
                                              extracted_outs['cluster_inds'], img_metas, rescale=rescale,
                                              iou_logits=outs.get('iou_logits', None))
        if self.as_rpn:
            return dict(all_input_points=dict_to_sample['seg_points'], valid_pts_feats=extracted_outs['cluster_pts_feats'],
                        valid_pts_xyz=extracted_outs['cluster_pts_xyz'], seg_feats=dict_to_sample['seg_feats'],
                        pts_mask=sampled_out['fg_mask_list'], pts_batch_inds=dict_to_sample['batch_idx'],
                        proposal_list=bbox_list)
        return [bbox3d2result(bboxes, scores, labels) for bboxes, scores, labels in bbox_list]


@DETECTORS.register_module()
class FSD(SingleStageFSD):
    """two_stage_fsd.py: + ``roi_head`` (GroupCorrectionHead); its DynamicPointROIExtractor is built, the box head not"""

    def __init__(self, backbone, segmentor, roi_head=None, **kw):
        super().__init__(backbone, segmentor, **kw)
        self.unbuilt['roi_head'] = roi_head
        ext = dict(_get(roi_head, 'roi_extractor', None) or {})
        self.with_virtual = ext.pop('with_virtual', False)
        self.roi_extractor = ROI_EXTRACTORS.build(ext) if ext else None

    def forward_train(self, points, img_metas, gt_bboxes_3d, gt_labels_3d, gt_bboxes_ignore=None):
        """two_stage_fsd.py:48-106: the first stage as RPN, its boxes as proposals, the RoI input, the RoI head's losses"""
        self._require_heads('forward_train')
        gt_bboxes_3d = [b[l >= 0] for b, l in zip(gt_bboxes_3d, gt_labels_3d)]
        gt_labels_3d = [l[l >= 0] for l in gt_labels_3d]
        point_drop_ratio = _get(self.train_cfg, 'point_drop_ratio', 0)
        if point_drop_ratio > 0:
            kept = []
            for p in points:
                idx = torch.randperm(len(p)).to(p.device)
                kept.append(p[idx[:int(len(p) * (1 - point_drop_ratio))]])
            points = kept
        losses = {}
        rpn_outs = super().forward_train(points=points, img_metas=img_metas, gt_bboxes_3d=gt_bboxes_3d,
                                         gt_labels_3d=gt_labels_3d, gt_bboxes_ignore=gt_bboxes_ignore,
                                         runtime_info=self.runtime_info)
        losses.update(rpn_outs['rpn_losses'])
        proposal_list = self.bbox_head.get_bboxes(rpn_outs['cls_logits'], rpn_outs['reg_preds'], rpn_outs['cluster_xyz'],
                                                  rpn_outs['cluster_inds'], img_metas)
        assert len(proposal_list) == len(gt_bboxes_3d)
        pts_xyz, pts_feats, pts_batch_inds = self.prepare_multi_class_roi_input(
            rpn_outs['all_input_points'], rpn_outs['valid_pts_feats'], rpn_outs['seg_feats'], rpn_outs['pts_mask'],
            rpn_outs['pts_batch_inds'], rpn_outs['valid_pts_xyz'])
        losses.update(self.roi_head.forward_train(pts_xyz, pts_feats, pts_batch_inds, img_metas, proposal_list, gt_bboxes_3d,
                                                  gt_labels_3d))
        return losses

    def _roi_detach(self):
        return dict(detach_seg_feats=bool(self.training and _get(self.train_cfg, 'detach_seg_feats', False)),
                    detach_cluster_feats=bool(self.training and _get(self.train_cfg, 'detach_cluster_feats', False)))

    def prepare_roi_input(self, points, cluster_pts_feats, pts_seg_feats, pts_mask, pts_batch_inds, cluster_pts_xyz):
        """two_stage_fsd.py:108-125 (one class: pad in place) over ``fg_sample.roi_input_single``; the reference's ``isclose``
        assert on the points (a device read) is dropped"""
        assert isinstance(pts_mask, list)
        return FS.roi_input_single(points, cluster_pts_feats, pts_seg_feats, pts_mask[:1], pts_batch_inds, **self._roi_detach())

    def prepare_multi_class_roi_input(self, points, cluster_pts_feats, pts_seg_feats, pts_mask, pts_batch_inds, cluster_pts_xyz):
        """two_stage_fsd.py:127-178 over ``fg_sample.roi_input``: rows sorted by sample, inside a sample the background points
        in point order, then class 0, class 1, ... (the stable sort of the reference's concatenation; the reference's
        ``sort()`` leaves that order open on a GPU).  One host read (the row count); the ``isclose`` assert is dropped."""
        assert isinstance(pts_mask, list)
        pts, feats, bidx, _ = FS.roi_input(points, cluster_pts_feats, pts_seg_feats, pts_mask, pts_batch_inds,
                                           self._num_samples(pts_batch_inds), **self._roi_detach())
        return pts, feats, bidx

    def simple_test(self, points, img_metas, imgs=None, rescale=False, gt_bboxes_3d=None, gt_labels_3d=None):
        """two_stage_fsd.py:180-223"""
        self._require_heads('simple_test')
        rpn_outs = super().simple_test(points=points, img_metas=img_metas, gt_bboxes_3d=gt_bboxes_3d, gt_labels_3d=gt_labels_3d)
        proposal_list = rpn_outs['proposal_list']
        if _get(self.test_cfg, 'skip_rcnn', False):
            return [bbox3d2result(bboxes, scores, labels) for bboxes, scores, labels in proposal_list]
        if self.num_classes > 1 or _get(self.test_cfg, 'enable_multi_class_test', False):
            prepare_func = self.prepare_multi_class_roi_input
        else:
            prepare_func = self.prepare_roi_input
        pts_xyz, pts_feats, pts_batch_inds = prepare_func(
            rpn_outs['all_input_points'], rpn_outs['valid_pts_feats'], rpn_outs['seg_feats'], rpn_outs['pts_mask'],
            rpn_outs['pts_batch_inds'], rpn_outs['valid_pts_xyz'])
        return self.roi_head.simple_test(pts_xyz, pts_feats, pts_batch_inds, img_metas, proposal_list, gt_bboxes_3d, gt_labels_3d)


@DETECTORS.register_module()
class SingleStageFSDV2(_HotPathDetector, VirtualVoxelExtractor):
    """segmentor (with multi-scale decoder features) -> (sampling) -> the virtual-voxel stage
    (single_stage_fsd_v2.py:38-271, 375-433; the stage: sst_amd/virtual_voxel.py - ``extract_feat`` is its forward)."""

    def __init__(self, backbone, segmentor, voxel_layer=None, voxel_encoder=None, middle_encoder=None, neck=None,
                 virtual_point_projector=None, pre_voxel_encoder=None, bbox_head=None, train_cfg=None, test_cfg=None,
                 pretrained=None, init_cfg=None, multiscale_cfg=None):
        VirtualVoxelExtractor.__init__(self, backbone, voxel_encoder, virtual_point_projector, train_cfg=train_cfg,
                                       test_cfg=test_cfg, multiscale_cfg=multiscale_cfg, bbox_head=bbox_head)
        self._init_common(segmentor, bbox_head, train_cfg or {}, test_cfg or {}, neck=neck, pre_voxel_encoder=pre_voxel_encoder)
        if voxel_layer is not None:
            self.voxel_layer = Voxelization(**voxel_layer)
        if middle_encoder is not None:
            self.middle_encoder = build_middle_encoder(middle_encoder)
        self.use_multiscale_features = self.segmentor.use_multiscale_features

    forward = VirtualVoxelExtractor.extract_feat


@DETECTORS.register_module()
class FSDV2(SingleStageFSDV2):
    """two_stage_fsd_v2.py:11-60: + ``roi_head``; the point RoI extractor is built (the SIR layers of its box head are
    sst_amd.SIRLayer, constructed by whoever builds that head)"""

    def __init__(self, backbone, segmentor, roi_head=None, **kw):
        super().__init__(backbone, segmentor, **kw)
        self.unbuilt['roi_head'] = roi_head
        ext = dict(_get(roi_head, 'roi_extractor', None) or {})
        self.with_virtual = ext.pop('with_virtual', False)
        self.roi_extractor = ROI_EXTRACTORS.build(ext) if ext else None
