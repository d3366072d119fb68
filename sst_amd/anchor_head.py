"""Anchor3DHead with its anchor generators, and the neck SECONDFPN (csrc/anchor_head.hip).

Reference: mmdet3d/models/dense_heads/anchor3d_head.py (forward :147-175, loss / loss_single / add_sin_difference :197-379,
get_bboxes / get_bboxes_single :381-551), train_mixins.py (anchor_target_3d :11-99, anchor_target_3d_single :101-235,
anchor_target_single_assigner :237-314, get_direction_target :317-346), mmdet3d/core/anchor/anchor_3d_generator.py
(Anchor3DRangeGenerator :8-209, AlignedAnchor3DRangeGenerator :212-325), mmdet3d/models/necks/second_fpn.py.

``anchor_targets``: one memset and two launches assign every anchor of the batch, for all anchor sizes, instead of the
reference's per-sample, per-size dense [G, H * W * n_rot] IoU matrices; the result is one int32 per anchor.  ``anchor_loss``: two
launches forward and one backward read the three NCHW maps where they lie and form the targets of the positive anchors in the
kernel; nothing is read back and no dense target tensor exists.  ``anchor_decode``: one launch per sample after torch.topk.  The
kernels never read an anchor tensor: an anchor is (cell, size index, rotation index) and its centre comes from the generator's
per-axis tables (``AnchorGrid``).  The three 1 x 1 convolutions and the neck are torch's.  fp32 device tensors only; CPU tensors
raise.
"""
import ctypes

import numpy as np
import torch
from torch import nn

from . import _lib
from . import box_ops
from . import roi_head  # noqa: F401  (registers DeltaXYZWLHRBBoxCoder)
from ._head_common import cfg_get as _get
from .center_head import build_bbox_coder
from .detectors import HEADS, NECKS
from .norm import build_conv_layer, build_norm_layer
from .registry import Registry

ANCHOR_GENERATORS = Registry('anchor generator')  # mmdet.core.anchor.ANCHOR_GENERATORS
MAX_SIZES, MAX_ROTS = 8, 4                         # SST_ANCHOR_MAX_SIZES, SST_ANCHOR_MAX_ROTS


def build_anchor_generator(cfg):
    return ANCHOR_GENERATORS.build(cfg)


def limit_period(val, offset=0.5, period=np.pi):
    """mmdet3d/core/bbox/structures/utils.py:7-21"""
    return val - torch.floor(val / period + offset) * period


def targets_gt_chunk():
    """ground-truth boxes per LDS pass of the assignment kernels"""
    return int(_lib.load().sst_anchor_targets_gt_chunk())


def block_cells():
    """cells per workgroup of the assignment and loss kernels"""
    return int(_lib.load().sst_anchor_block())


class AnchorGrid(object):
    """the anchors of one feature-map size as the kernels see them: the centre tables on the device (xs [n_sizes, W], ys
    [n_sizes, H], zs [n_sizes] in one tensor) and the sizes and rotations that travel as kernel arguments"""

    def __init__(self, centers, height, width, sizes, rotations):
        self.centers, self.H, self.W = centers, int(height), int(width)
        self.sizes = [[float(v) for v in s] for s in sizes]       # fp32 values
        self.rotations = [float(r) for r in rotations]
        self.n_sizes, self.n_rots = len(self.sizes), len(self.rotations)
        if self.n_sizes > MAX_SIZES or self.n_rots > MAX_ROTS:
            raise NotImplementedError(f'anchor_generator: at most {MAX_SIZES} sizes and {MAX_ROTS} rotations are built, got '
                                      f'{self.n_sizes} and {self.n_rots}')
        c = _lib.AnchorGrid()
        c.centers = centers.data_ptr()
        c.H, c.W, c.n_sizes, c.n_rots = self.H, self.W, self.n_sizes, self.n_rots
        for i, s in enumerate(self.sizes):
            for k in range(3):
                c.sizes[i][k] = s[k]
        for i, r in enumerate(self.rotations):
            c.rots[i] = r
        self.c = c

    num_base_anchors = property(lambda self: self.n_sizes * self.n_rots)
    num_anchors = property(lambda self: self.H * self.W * self.n_sizes * self.n_rots)
    xs = property(lambda self: self.centers[:self.n_sizes * self.W].view(self.n_sizes, self.W))
    ys = property(lambda self: self.centers[self.n_sizes * self.W:self.n_sizes * (self.W + self.H)].view(self.n_sizes, self.H))
    zs = property(lambda self: self.centers[self.n_sizes * (self.W + self.H):])

    def ref(self):
        return ctypes.byref(self.c)

    def anchors(self):
        """the reference's [1, H, W, n_sizes, n_rots, 7] tensor (for callers and tests; the kernels do not read it)"""
        dev, shape = self.centers.device, (1, self.H, self.W, self.n_sizes, self.n_rots)
        x = self.xs.t().reshape(1, 1, self.W, self.n_sizes, 1).expand(shape)
        y = self.ys.t().reshape(1, self.H, 1, self.n_sizes, 1).expand(shape)
        z = self.zs.reshape(1, 1, 1, self.n_sizes, 1).expand(shape)
        size = torch.tensor(self.sizes, dtype=torch.float32, device=dev).reshape(1, 1, 1, self.n_sizes, 1, 3)
        rot = torch.tensor(self.rotations, dtype=torch.float32, device=dev).reshape(1, 1, 1, 1, self.n_rots).expand(shape)
        return torch.cat([x.unsqueeze(-1), y.unsqueeze(-1), z.unsqueeze(-1), size.expand(*shape, 3), rot.unsqueeze(-1)], -1)


@ANCHOR_GENERATORS.register_module()
class Anchor3DRangeGenerator(object):
    """core/anchor/anchor_3d_generator.py:8-209: centres spread uniformly between the ends of the range"""

    def __init__(self, ranges, sizes=[[1.6, 3.9, 1.56]], scales=[1], rotations=[0, 1.5707963], custom_values=(),
                 reshape_out=True, size_per_range=True):
        assert isinstance(ranges, (list, tuple)) and all(isinstance(r, (list, tuple)) for r in ranges)
        if size_per_range:
            if len(sizes) != len(ranges):
                assert len(ranges) == 1
                ranges = list(ranges) * len(sizes)
            assert len(ranges) == len(sizes)
        else:
            assert len(ranges) == 1
        assert isinstance(scales, list)
        if len(custom_values) > 0:
            raise NotImplementedError(f'anchor_generator: custom_values {custom_values} (box codes above 7) are not built')
        self.sizes, self.scales, self.ranges, self.rotations = sizes, scales, ranges, rotations
        self.custom_values = custom_values
        self.reshape_out, self.size_per_range = reshape_out, size_per_range
        self._grids = {}

    def __repr__(self):
        return (f'{self.__class__.__name__}(anchor_range={self.ranges},\nscales={self.scales},\nsizes={self.sizes},\n'
                f'rotations={self.rotations},\nreshape_out={self.reshape_out},\nsize_per_range={self.size_per_range})')

    @property
    def num_base_anchors(self):
        return len(self.rotations) * torch.tensor(self.sizes).reshape(-1, 3).size(0)

    @property
    def num_levels(self):
        return len(self.scales)

    def _axis(self, lo, hi, n, device):
        """the centres of one axis of one range, the reference's arithmetic on ``device``"""
        return torch.linspace(lo, hi, n, device=device)

    def grid(self, featmap_size, device, level=0):
        """-> AnchorGrid of one level, formed once per (feature-map size, device) and kept"""
        height, width = int(featmap_size[-2]), int(featmap_size[-1])
        depth = int(featmap_size[0]) if len(featmap_size) == 3 else 1
        if depth != 1:
            raise NotImplementedError('anchor_generator: feature maps of more than one z layer are not built')
        key = (height, width, str(torch.device(device)), level)
        if key not in self._grids:
            pairs = []      # (range, [n, 3] sizes) in the order of the anchors' size axis
            if self.size_per_range:
                for rng, size in zip(self.ranges, self.sizes):
                    pairs.append((rng, torch.tensor(size, dtype=torch.float32).reshape(-1, 3) * self.scales[level]))
            else:
                pairs.append((self.ranges[0], torch.tensor(self.sizes, dtype=torch.float32).reshape(-1, 3) * self.scales[level]))
            xs, ys, zs, sizes = [], [], [], []
            for rng, size in pairs:
                r = torch.tensor(rng, dtype=torch.float32)     # the reference's fp32 tensor of the range, read back as scalars
                x = self._axis(r[0].item(), r[3].item(), width, device)
                y = self._axis(r[1].item(), r[4].item(), height, device)
                z = self._axis(r[2].item(), r[5].item(), 1, device)
                for row in size.tolist():
                    xs.append(x)
                    ys.append(y)
                    zs.append(z)
                    sizes.append(row)
            centers = torch.cat(xs + ys + zs).contiguous()
            rots = torch.tensor(self.rotations, dtype=torch.float32).tolist()
            self._grids[key] = AnchorGrid(centers, height, width, sizes, rots)
        return self._grids[key]

    def grid_anchors(self, featmap_sizes, device='cuda'):
        assert self.num_levels == len(featmap_sizes)
        out = []
        for i in range(self.num_levels):
            anchors = self.grid(featmap_sizes[i], device, i).anchors()
            out.append(anchors.reshape(-1, anchors.size(-1)) if self.reshape_out else anchors)
        return out


@ANCHOR_GENERATORS.register_module()
class AlignedAnchor3DRangeGenerator(Anchor3DRangeGenerator):
    """core/anchor/anchor_3d_generator.py:212-325: centres on the cells of the feature grid"""

    def __init__(self, align_corner=False, **kwargs):
        super().__init__(**kwargs)
        self.align_corner = align_corner

    def _axis(self, lo, hi, n, device):
        centers = torch.linspace(lo, hi, n + 1, device=device)
        if not self.align_corner:
            centers += (centers[1] - centers[0]) / 2
        return centers[:n]


class AnchorTargets(object):
    """the compact result of ``anchor_targets``: ``assigned`` int32 [B, A] (box index within the sample, -1 background, -2
    ignored; A in the reference's (h, w, size, rot) order), the concatenated ``gt_boxes`` [G, cols] / ``gt_labels`` int64 [G]
    with ``gt_offsets`` (device int32 [B + 1]; ``offsets`` the same as a Python list), ``pos_counts`` int32 [B] on the device and
    ``gt_max`` fp32 [n_sizes, G], the largest IoU of every box over the anchors of each size"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _parse_assigners(assigner, n_sizes):
    """the config's MaxIoUAssigner dict(s) -> (pos_iou_thr, neg_iou_thr, min_pos_iou) per size; refuses by name"""
    cfgs = list(assigner) if isinstance(assigner, (list, tuple)) else [assigner] * n_sizes
    if len(cfgs) != n_sizes:
        raise RuntimeError(f'Anchor3DHead: {len(cfgs)} assigners for {n_sizes} anchor sizes')
    pos, neg, low = [], [], []
    for c in cfgs:
        if _get(c, 'type') != 'MaxIoUAssigner':
            raise NotImplementedError(f'assigner type {_get(c, "type")!r}: only MaxIoUAssigner is built')
        calc = _get(c, 'iou_calculator', dict(type='BboxOverlaps2D'))
        if _get(calc, 'type') != 'BboxOverlapsNearest3D' or _get(calc, 'coordinate', 'lidar') != 'lidar':
            raise NotImplementedError(f'iou_calculator {dict(calc)}: only BboxOverlapsNearest3D(\'lidar\') is built')
        if _get(c, 'ignore_iof_thr', -1) > 0:
            raise NotImplementedError(f'ignore_iof_thr {_get(c, "ignore_iof_thr")} > 0 is not built')
        for key in ('match_low_quality', 'gt_max_assign_all'):
            if not _get(c, key, True):
                raise NotImplementedError(f'{key}=False is not built')
        if _get(c, 'gpu_assign_thr', -1) > 0:
            raise NotImplementedError('gpu_assign_thr > 0 is not built')
        if not isinstance(_get(c, 'neg_iou_thr'), (int, float)):
            raise NotImplementedError(f'neg_iou_thr {_get(c, "neg_iou_thr")!r}: only a single number is built')
        if not _get(c, 'min_pos_iou', 0.0) > 0:
            raise NotImplementedError(f'min_pos_iou {_get(c, "min_pos_iou", 0.0)} <= 0 is not built')
        if not _get(c, 'pos_iou_thr') > 0:
            raise NotImplementedError(f'pos_iou_thr {_get(c, "pos_iou_thr")} <= 0 is not built')
        pos.append(float(c['pos_iou_thr']))
        neg.append(float(c['neg_iou_thr']))
        low.append(float(c['min_pos_iou']))
    return pos, neg, low


@torch.no_grad()
def anchor_targets(gt_bboxes_list, gt_labels_list, featmap_size, anchor_generator, assigner, assign_per_class=False):
    """-> AnchorTargets for the whole batch and every anchor size: one memset and two launches, nothing is read back.

    gt_bboxes_list: per sample a [G_i, >= 7] fp32 device tensor (x, y, z_bottom, w, l, h, rz, ...) or an object with ``.tensor``;
    gt_labels_list: [G_i] integer device tensors; featmap_size (H, W); anchor_generator: a generator of this module (or an
    AnchorGrid); assigner: the config's MaxIoUAssigner dict, or the list of them with one per anchor size.  With
    ``assign_per_class`` the anchors of size i meet the boxes of label i only.  Labels outside [0, num_classes) are outside the
    contract: such a box still takes part in the assignment (as in the reference) and its anchors get no class target."""
    if len(gt_bboxes_list) != len(gt_labels_list) or len(gt_bboxes_list) == 0:
        raise RuntimeError('anchor_targets: one box set and one label set per sample expected')
    boxes_list = [b.tensor if hasattr(b, 'tensor') else b for b in gt_bboxes_list]
    for b, l in zip(boxes_list, gt_labels_list):
        _lib.require_cuda(b.contiguous(), l.contiguous())
        if b.dtype != torch.float32 or b.dim() != 2 or l.numel() != b.size(0) or (b.size(0) and b.size(1) < 7):
            raise RuntimeError(f'anchor_targets: fp32 boxes [G, >= 7] and G labels expected, got {b.dtype} {tuple(b.shape)}, '
                               f'{tuple(l.shape)}')
    dev = boxes_list[0].device
    grid = anchor_generator if isinstance(anchor_generator, AnchorGrid) else anchor_generator.grid(featmap_size, dev)
    if (grid.H, grid.W) != (int(featmap_size[-2]), int(featmap_size[-1])) or grid.centers.device != dev:
        raise RuntimeError('anchor_targets: the anchor grid is of another feature-map size or device')
    pos, neg, low = _parse_assigners(assigner, grid.n_sizes)
    cols = {b.size(1) for b in boxes_list if b.size(0)}
    if len(cols) > 1:
        raise RuntimeError(f'anchor_targets: boxes of one width expected, got {sorted(cols)}')
    cols = cols.pop() if cols else 7
    filled = [b for b in boxes_list if b.size(0)]
    boxes = torch.cat(filled, 0).contiguous() if filled else torch.zeros((0, cols), dtype=torch.float32, device=dev)
    labels = torch.cat([l.reshape(-1).to(device=dev, dtype=torch.long) for l in gt_labels_list]).contiguous()
    off = [0]
    for b in boxes_list:
        off.append(off[-1] + b.size(0))
    gt_offsets = torch.tensor(off, dtype=torch.int32).to(dev, non_blocking=True)
    batch, n_gts = len(boxes_list), boxes.size(0)
    assigned = torch.empty((batch, grid.num_anchors), dtype=torch.int32, device=dev)
    state = torch.empty(grid.n_sizes * n_gts + batch, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().sst_anchor_targets_f32(
        grid.ref(), _lib.ptr(boxes), cols, _lib.ptr(labels), _lib.ptr(gt_offsets), n_gts, batch, 1 if assign_per_class else 0,
        _lib.farray(pos), _lib.farray(neg), _lib.farray(low), _lib.ptr(assigned), _lib.ptr(state), _lib.stream_ptr()),
        'sst_anchor_targets_f32')
    return AnchorTargets(assigned=assigned, gt_boxes=boxes, gt_labels=labels, gt_offsets=gt_offsets, offsets=off,
                         pos_counts=state[grid.n_sizes * n_gts:],
                         gt_max=state[:grid.n_sizes * n_gts].view(torch.float32).view(grid.n_sizes, n_gts), grid=grid)


def _loss_args(cls_score, bbox_pred, dir_cls_preds, targets, cfg):
    a = _lib.AnchorLossArgs()
    a.cls_score, a.bbox_pred = cls_score.data_ptr(), bbox_pred.data_ptr()
    a.dir_pred = None if dir_cls_preds is None else dir_cls_preds.data_ptr()
    a.assigned = targets.assigned.data_ptr()
    a.gts = targets.gt_boxes.data_ptr() if targets.gt_boxes.size(0) else None
    a.gt_labels = targets.gt_labels.data_ptr() if targets.gt_boxes.size(0) else None
    a.gt_offsets, a.pos_counts = targets.gt_offsets.data_ptr(), targets.pos_counts.data_ptr()
    a.n_gts, a.gt_cols, a.batch = targets.gt_boxes.size(0), targets.gt_boxes.size(1), cls_score.size(0)
    a.num_classes = cfg['num_classes']
    a.smooth_l1, a.sin_diff = (1 if cfg['smooth_l1'] else 0), (1 if cfg['sin_diff'] else 0)
    for k in ('gamma', 'alpha', 'w_cls', 'w_bbox', 'w_dir', 'beta', 'pos_weight', 'dir_offset'):
        setattr(a, k, float(cfg[k]))
    for i, v in enumerate(cfg['code_weight']):
        a.code_weight[i] = float(v)
    return a


class _AnchorLoss(torch.autograd.Function):

    @staticmethod
    def forward(ctx, cls_score, bbox_pred, dir_cls_preds, targets, cfg):
        lib, dev, grid = _lib.load(), cls_score.device, targets.grid
        out = torch.empty(4, dtype=torch.float32, device=dev)
        ws = _lib.workspace(lib.sst_anchor_loss_workspace_bytes(cls_score.size(0), grid.H, grid.W), dev)
        args = _loss_args(cls_score, bbox_pred, dir_cls_preds, targets, cfg)
        _lib.check(lib.sst_anchor_loss_fwd_f32(grid.ref(), ctypes.byref(args), _lib.ptr(out), _lib.ptr(ws), _lib.stream_ptr()),
                   'sst_anchor_loss_fwd_f32')
        ctx.save_for_backward(cls_score, bbox_pred, out, *([] if dir_cls_preds is None else [dir_cls_preds]))
        ctx.targets, ctx.cfg = targets, cfg
        ctx.set_materialize_grads(False)      # a loss nobody differentiates arrives as None: the kernel writes its zeros
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_cls, g_box, g_dir):
        cls_score, bbox_pred, out = ctx.saved_tensors[:3]
        dir_cls_preds = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
        g_cls, g_box, g_dir = (None if g is None else g.to(torch.float32).contiguous() for g in (g_cls, g_box, g_dir))
        d_cls, d_box = torch.empty_like(cls_score), torch.empty_like(bbox_pred)
        d_dir = None if dir_cls_preds is None else torch.empty_like(dir_cls_preds)
        args = _loss_args(cls_score, bbox_pred, dir_cls_preds, ctx.targets, ctx.cfg)
        _lib.check(_lib.load().sst_anchor_loss_bwd_f32(
            ctx.targets.grid.ref(), ctypes.byref(args), _lib.ptr(out), _lib.ptr(g_cls), _lib.ptr(g_box), _lib.ptr(g_dir),
            _lib.ptr(d_cls), _lib.ptr(d_box), _lib.ptr(d_dir), _lib.stream_ptr()), 'sst_anchor_loss_bwd_f32')
        return d_cls, d_box, d_dir, None, None


def anchor_loss(cls_score, bbox_pred, dir_cls_preds, targets, num_classes, gamma=2.0, alpha=0.25, loss_weight_cls=1.0,
                smooth_l1_beta=None, loss_weight_bbox=1.0, loss_weight_dir=1.0, code_weight=None, diff_rad_by_sin=True,
                dir_offset=0.0, pos_weight=-1):
    """-> (loss_cls, loss_bbox, loss_dir) of Anchor3DHead.loss_single, each 'mean' with avg_factor = sum over the samples of
    max(positives, 1), which stays on the device.

    cls_score [B, n_a * C, H, W], bbox_pred [B, n_a * 7, H, W], dir_cls_preds [B, n_a * 2, H, W] or None (then loss_dir is 0):
    the head's raw outputs, read where they lie; targets: the AnchorTargets of the same feature-map size.
      loss_cls  = loss_weight_cls * sum(weight * sigmoid focal loss(gamma, alpha)) / avg_factor, weight 0 on ignored anchors,
                  pos_weight (when > 0) on positives, 1 elsewhere
      loss_bbox = loss_weight_bbox * sum over positives of (|d| or smooth L1(beta)) * code_weight / avg_factor, d = prediction -
                  DeltaXYZWLHRBBoxCoder.encode(anchor, box), the yaw term through add_sin_difference when ``diff_rad_by_sin``
      loss_dir  = loss_weight_dir * sum over positives of the 2-way cross entropy against get_direction_target / avg_factor
    Without a positive in the batch loss_bbox and loss_dir are 0 and carry zero gradients."""
    maps = [cls_score, bbox_pred] + ([] if dir_cls_preds is None else [dir_cls_preds])
    _lib.require_cuda(*maps)
    grid = targets.grid
    n_a = grid.num_base_anchors
    b = cls_score.size(0) if cls_score.dim() == 4 else -1
    for name, t, c in zip(('cls_score', 'bbox_pred', 'dir_cls_preds'), maps, (num_classes, 7, 2)):
        if t.dtype != torch.float32:
            raise RuntimeError(f'anchor_loss: float32 tensors expected, got {t.dtype}')
        if tuple(t.shape) != (b, n_a * c, grid.H, grid.W):
            raise RuntimeError(f'anchor_loss: {name} must be [B, {n_a * c}, {grid.H}, {grid.W}], got {tuple(t.shape)}')
    if tuple(targets.assigned.shape) != (b, grid.num_anchors):
        raise RuntimeError('anchor_loss: the targets are of another batch or feature-map size')
    code_weight = [1.0] * 7 if not code_weight else [float(v) for v in code_weight]
    if len(code_weight) != 7:
        raise RuntimeError('anchor_loss: seven code weights expected')
    cfg = dict(num_classes=int(num_classes), gamma=gamma, alpha=alpha, w_cls=loss_weight_cls, w_bbox=loss_weight_bbox,
               w_dir=loss_weight_dir, smooth_l1=smooth_l1_beta is not None, beta=smooth_l1_beta or 0.0, sin_diff=diff_rad_by_sin,
               dir_offset=dir_offset, pos_weight=pos_weight, code_weight=code_weight)
    return _AnchorLoss.apply(cls_score, bbox_pred, dir_cls_preds, targets, cfg)


@torch.no_grad()
def anchor_decode(cls_score, bbox_pred, dir_cls_pred, grid, num_classes, inds=None):
    """one sample: -> (boxes [n, 7], scores [n, C + 1] with the zero background column, dir int64 [n], bev xyxyr [n, 5]) of the
    anchors ``inds`` (int64 [n], the reference's (h, w, size, rot) order; None: all of them).  cls_score [n_a * C, H, W],
    bbox_pred [n_a * 7, H, W], dir_cls_pred [n_a * 2, H, W] or None: contiguous maps of the sample."""
    maps = [cls_score, bbox_pred] + ([] if dir_cls_pred is None else [dir_cls_pred])
    _lib.require_cuda(*maps, inds)
    n_a = grid.num_base_anchors
    for t, c in zip(maps, (num_classes, 7, 2)):
        if t.dtype != torch.float32 or tuple(t.shape) != (n_a * c, grid.H, grid.W):
            raise RuntimeError(f'anchor_decode: fp32 [{n_a * c}, {grid.H}, {grid.W}] expected, got {t.dtype} {tuple(t.shape)}')
    if inds is not None and inds.dtype != torch.long:
        raise RuntimeError('anchor_decode: int64 indices expected')
    n, dev = (grid.num_anchors if inds is None else inds.numel()), cls_score.device
    boxes = torch.empty((n, 7), dtype=torch.float32, device=dev)
    scores = torch.empty((n, num_classes + 1), dtype=torch.float32, device=dev)
    dirs = torch.empty(n, dtype=torch.long, device=dev)
    bev = torch.empty((n, 5), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().sst_anchor_decode_f32(
        grid.ref(), _lib.ptr(cls_score), _lib.ptr(bbox_pred), _lib.ptr(dir_cls_pred), _lib.ptr(inds), n, int(num_classes),
        _lib.ptr(boxes), _lib.ptr(scores), _lib.ptr(dirs), _lib.ptr(bev), _lib.stream_ptr()), 'sst_anchor_decode_f32')
    return boxes, scores, dirs, bev


@HEADS.register_module()
class Anchor3DHead(nn.Module):
    """Anchor3DHead (dense_heads/anchor3d_head.py): the reference's constructor arguments, submodule names and initialisation;
    targets, losses and box extraction on the kernels of csrc/anchor_head.hip.  What the kernels do not cover is refused by name:
    at construction, or where the key is first used (``get_bboxes`` for the ``test_cfg``)."""

    def __init__(self, num_classes, in_channels, train_cfg, test_cfg, feat_channels=256, use_direction_classifier=True,
                 anchor_generator=dict(type='Anchor3DRangeGenerator', range=[0, -39.68, -1.78, 69.12, 39.68, -1.78], strides=[2],
                                       sizes=[[1.6, 3.9, 1.56]], rotations=[0, 1.57], custom_values=[], reshape_out=False),
                 assigner_per_size=False, assign_per_class=False, diff_rad_by_sin=True, dir_offset=0, dir_limit_offset=1,
                 bbox_coder=dict(type='DeltaXYZWLHRBBoxCoder'),
                 loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                 loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=2.0),
                 loss_dir=dict(type='CrossEntropyLoss', loss_weight=0.2), init_cfg=None):
        super().__init__()
        self.in_channels, self.num_classes, self.feat_channels = in_channels, num_classes, feat_channels
        self.diff_rad_by_sin, self.use_direction_classifier = diff_rad_by_sin, use_direction_classifier
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.assigner_per_size, self.assign_per_class = assigner_per_size, assign_per_class
        self.dir_offset, self.dir_limit_offset = dir_offset, dir_limit_offset
        self.fp16_enabled = False
        if assigner_per_size:
            raise NotImplementedError('Anchor3DHead: assigner_per_size=True is not built')
        self.anchor_generator = build_anchor_generator(anchor_generator)
        if self.anchor_generator.num_levels != 1:
            raise NotImplementedError(f'Anchor3DHead: anchor_generator scales {self.anchor_generator.scales}: more than one '
                                      'feature level is not built')
        self.num_anchors = self.anchor_generator.num_base_anchors
        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.box_code_size = self.bbox_coder.code_size
        if _get(bbox_coder, 'type') != 'DeltaXYZWLHRBBoxCoder' or self.box_code_size != 7:
            raise NotImplementedError(f'Anchor3DHead: bbox_coder {dict(bbox_coder)}: only DeltaXYZWLHRBBoxCoder with code_size 7 '
                                      'is built')
        self.use_sigmoid_cls = loss_cls.get('use_sigmoid', False)
        self.sampling = loss_cls['type'] not in ['FocalLoss', 'GHMC']
        if loss_cls.get('type') != 'FocalLoss' or loss_cls.get('reduction', 'mean') != 'mean':
            raise NotImplementedError(f'Anchor3DHead: loss_cls {dict(loss_cls)}: only FocalLoss (mean) with the PseudoSampler is '
                                      'built')
        if not self.use_sigmoid_cls:
            raise NotImplementedError('Anchor3DHead: loss_cls use_sigmoid=False (softmax class scores) is not built')
        if loss_bbox.get('type') not in ('L1Loss', 'SmoothL1Loss') or loss_bbox.get('reduction', 'mean') != 'mean':
            raise NotImplementedError(f'Anchor3DHead: loss_bbox {dict(loss_bbox)}: only L1Loss and SmoothL1Loss (mean) are built')
        if use_direction_classifier and (loss_dir.get('type') != 'CrossEntropyLoss' or loss_dir.get('use_sigmoid', False)
                                         or loss_dir.get('use_mask', False) or loss_dir.get('class_weight') is not None
                                         or loss_dir.get('reduction', 'mean') != 'mean'):
            raise NotImplementedError(f'Anchor3DHead: loss_dir {dict(loss_dir)}: only the softmax CrossEntropyLoss (mean) is built')
        self.loss_cfg = dict(loss_cls=dict(loss_cls), loss_bbox=dict(loss_bbox), loss_dir=dict(loss_dir))
        self.smooth_l1_beta = float(loss_bbox.get('beta', 1.0)) if loss_bbox['type'] == 'SmoothL1Loss' else None
        if train_cfg is not None:
            n_sizes = self.num_anchors // len(self.anchor_generator.rotations)
            _parse_assigners(_get(train_cfg, 'assigner'), n_sizes)

        self.cls_out_channels = self.num_anchors * self.num_classes
        self.conv_cls = nn.Conv2d(self.feat_channels, self.cls_out_channels, 1)
        self.conv_reg = nn.Conv2d(self.feat_channels, self.num_anchors * self.box_code_size, 1)
        if self.use_direction_classifier:
            self.conv_dir_cls = nn.Conv2d(self.feat_channels, self.num_anchors * 2, 1)
        self.init_cfg = init_cfg if init_cfg is not None else dict(
            type='Normal', layer='Conv2d', std=0.01, override=dict(type='Normal', name='conv_cls', std=0.01, bias_prob=0.01))
        self.init_weights()

    def init_weights(self):
        """the reference's default init_cfg: Normal(std 0.01) on the convolutions, conv_cls' bias from bias_prob 0.01"""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.constant_(m.bias, 0)
        nn.init.constant_(self.conv_cls.bias, float(-np.log((1 - 0.01) / 0.01)))

    def forward_single(self, x):
        cls_score = self.conv_cls(x)
        bbox_pred = self.conv_reg(x)
        dir_cls_preds = self.conv_dir_cls(x) if self.use_direction_classifier else None
        return cls_score, bbox_pred, dir_cls_preds

    def forward(self, feats):
        self._one_level(feats)
        return tuple(map(list, zip(*map(self.forward_single, feats))))

    @staticmethod
    def _one_level(maps):
        if len(maps) != 1:
            raise NotImplementedError(f'Anchor3DHead: {len(maps)} feature levels: more than one feature level is not built')

    def get_anchors(self, featmap_sizes, input_metas, device='cuda'):
        multi_level_anchors = self.anchor_generator.grid_anchors(featmap_sizes, device=device)
        return [multi_level_anchors for _ in range(len(input_metas))]

    def targets(self, gt_bboxes, gt_labels, featmap_size):
        """-> AnchorTargets (``anchor_targets`` with the head's generator and assigners)"""
        return anchor_targets(gt_bboxes, gt_labels, featmap_size, self.anchor_generator, _get(self.train_cfg, 'assigner'),
                              self.assign_per_class)

    @torch.no_grad()
    def anchor_target_3d(self, anchor_list, gt_bboxes_list, input_metas, gt_bboxes_ignore_list=None, gt_labels_list=None,
                         label_channels=1, num_classes=1, sampling=True, featmap_size=None):
        """-> (labels_list, label_weights_list, bbox_targets_list, bbox_weights_list, dir_targets_list, dir_weights_list,
        num_total_pos, num_total_neg) as the reference returns them, expanded from the compact targets with torch ops.  For API
        compatibility and tests: ``loss`` does not come through here, and this is the only place that reads the counts back.
        The feature-map size is taken from the anchors' shape ([1, H, W, n_sizes, n_rots, 7]) unless given."""
        if featmap_size is None:
            anchors = anchor_list[0][0]
            if anchors.dim() != 6:
                raise RuntimeError('anchor_target_3d: pass featmap_size with reshaped anchors')
            featmap_size = tuple(anchors.shape[1:3])
        if gt_labels_list is None:
            raise NotImplementedError('anchor_target_3d: gt_labels_list=None is not built')
        t = self.targets(gt_bboxes_list, gt_labels_list, featmap_size)
        grid, dev = t.grid, t.assigned.device
        batch, total = t.assigned.shape
        anchors = grid.anchors().reshape(1, total, 7)
        pos = t.assigned >= 0
        labels = torch.full((batch, total), num_classes, dtype=torch.long, device=dev)
        bbox_targets = torch.zeros((batch, total, 7), dtype=torch.float32, device=dev)
        dir_targets = torch.zeros((batch, total), dtype=torch.long, device=dev)
        if t.gt_boxes.size(0):
            first = torch.tensor(t.offsets[:-1], dtype=torch.long).to(dev).view(-1, 1)
            idx = (t.assigned.long().clamp(min=0) + first).clamp(max=t.gt_boxes.size(0) - 1)
            labels = torch.where(pos, t.gt_labels[idx], labels)
            enc = self.bbox_coder.encode(anchors.expand(batch, total, 7), t.gt_boxes[idx][..., :7])
            bbox_targets = torch.where(pos.unsqueeze(-1), enc, bbox_targets)
            offset_rot = limit_period(enc[..., 6] + anchors[..., 6] - self.dir_offset, 0, 2 * np.pi)
            dirs = torch.clamp(torch.floor(offset_rot / np.pi).long(), min=0, max=1)
            dir_targets = torch.where(pos, dirs, dir_targets)
        pos_f = pos.float()
        pos_weight = _get(self.train_cfg, 'pos_weight', -1)
        label_weights = torch.where(pos, pos_f * (1.0 if pos_weight <= 0 else float(pos_weight)), (t.assigned == -1).float())
        bbox_weights = pos_f.unsqueeze(-1).expand(batch, total, 7).contiguous()
        num_pos = t.pos_counts.tolist()
        num_neg = (t.assigned == -1).sum(1).tolist()
        return ([labels], [label_weights], [bbox_targets], [bbox_weights], [dir_targets], [pos_f.clone()],
                sum(max(n, 1) for n in num_pos), sum(max(n, 1) for n in num_neg))

    def loss(self, cls_scores, bbox_preds, dir_cls_preds, gt_bboxes, gt_labels, input_metas, gt_bboxes_ignore=None):
        """-> dict(loss_cls, loss_bbox, loss_dir), each a one-element list (one feature level), as the reference returns them"""
        self._one_level(cls_scores)
        cls_score, bbox_pred = _lib.as_fp32(cls_scores[0], bbox_preds[0])    # force_fp32
        dir_pred = _lib.as_fp32(dir_cls_preds[0]) if self.use_direction_classifier else None
        t = self.targets(gt_bboxes, gt_labels, tuple(cls_score.shape[-2:]))
        cfg = self.loss_cfg
        loss_cls, loss_bbox, loss_dir = anchor_loss(
            cls_score.contiguous(), bbox_pred.contiguous(), None if dir_pred is None else dir_pred.contiguous(), t,
            self.num_classes, gamma=cfg['loss_cls'].get('gamma', 2.0), alpha=cfg['loss_cls'].get('alpha', 0.25),
            loss_weight_cls=cfg['loss_cls'].get('loss_weight', 1.0), smooth_l1_beta=self.smooth_l1_beta,
            loss_weight_bbox=cfg['loss_bbox'].get('loss_weight', 1.0), loss_weight_dir=cfg['loss_dir'].get('loss_weight', 1.0),
            code_weight=_get(self.train_cfg, 'code_weight', None), diff_rad_by_sin=self.diff_rad_by_sin,
            dir_offset=self.dir_offset, pos_weight=_get(self.train_cfg, 'pos_weight', -1))
        return dict(loss_cls=[loss_cls], loss_bbox=[loss_bbox], loss_dir=[loss_dir if self.use_direction_classifier else None])

    def forward_train(self, feats, gt_bboxes_3d, gt_labels_3d, input_metas, gt_bboxes_ignore=None):
        outs = self(feats)
        return self.loss(*outs, gt_bboxes_3d, gt_labels_3d, input_metas, gt_bboxes_ignore=gt_bboxes_ignore)

    @torch.no_grad()
    def get_bboxes(self, cls_scores, bbox_preds, dir_cls_preds, input_metas, cfg=None, rescale=False):
        """-> per sample (boxes [n, 7] - wrapped by input_metas[i]['box_type_3d'] when given -, scores [n], labels int64 [n])"""
        self._one_level(cls_scores)
        cfg = self.test_cfg if cfg is None else cfg
        for key in ('wnms', 'wnms_gpu'):
            if _get(cfg, key, False):
                raise NotImplementedError(f'Anchor3DHead.get_bboxes: test_cfg {key}=True (weighted NMS) is not built')
        cls_score, bbox_pred = _lib.as_fp32(cls_scores[0].detach(), bbox_preds[0].detach())
        dir_pred = _lib.as_fp32(dir_cls_preds[0].detach()) if self.use_direction_classifier else None
        grid = self.anchor_generator.grid(tuple(cls_score.shape[-2:]), cls_score.device)
        return [self.get_bboxes_single(cls_score[i].contiguous(), bbox_pred[i].contiguous(),
                                       None if dir_pred is None else dir_pred[i].contiguous(), grid, input_metas[i], cfg)
                for i in range(len(input_metas))]

    def get_bboxes_single(self, cls_score, bbox_pred, dir_cls_pred, grid, input_meta, cfg):
        n_a, hw = grid.num_base_anchors, grid.H * grid.W
        nms_pre = _get(cfg, 'nms_pre', -1)
        inds = None
        if nms_pre > 0 and grid.num_anchors > nms_pre:
            # scores.max(dim=1) in the reference's (h, w, size, rot) order, then torch.topk: the selection stays torch's
            max_scores = cls_score.sigmoid().view(n_a, self.num_classes, hw).amax(1).t().reshape(-1)
            inds = max_scores.topk(nms_pre)[1].contiguous()
        boxes, scores, dirs, bev = anchor_decode(cls_score, bbox_pred, dir_cls_pred, grid, self.num_classes, inds)
        bboxes, scores, labels, dir_scores = box_ops.box3d_multiclass_nms(
            boxes, bev, scores, _get(cfg, 'score_thr', 0), _get(cfg, 'max_num'), cfg, dirs)
        if bboxes.shape[0] > 0:
            dir_rot = limit_period(bboxes[..., 6] - self.dir_offset, self.dir_limit_offset, np.pi)
            bboxes[..., 6] = dir_rot + self.dir_offset + np.pi * dir_scores.to(bboxes.dtype)
        box_type = (input_meta or {}).get('box_type_3d')
        if box_type is not None:
            bboxes = box_type(bboxes, box_dim=self.box_code_size)
        return bboxes, scores, labels


@NECKS.register_module()
class SECONDFPN(nn.Module):
    """necks/second_fpn.py: per input a deblock [ConvTranspose2d (or Conv2d for a stride of 1 with ``use_conv_for_no_stride``),
    norm, ReLU], outputs concatenated along the channels.  Plain torch; ``state_dict`` keys ``deblocks.N.M.*``."""

    def __init__(self, in_channels=[128, 128, 256], out_channels=[256, 256, 256], upsample_strides=[1, 2, 4],
                 norm_cfg=dict(type='BN', eps=1e-3, momentum=0.01), upsample_cfg=dict(type='deconv', bias=False),
                 conv_cfg=dict(type='Conv2d', bias=False), use_conv_for_no_stride=False, init_cfg=None):
        super().__init__()
        assert len(out_channels) == len(upsample_strides) == len(in_channels)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.fp16_enabled = False
        deblocks = []
        for i, out_channel in enumerate(out_channels):
            stride = upsample_strides[i]
            if stride > 1 or (stride == 1 and not use_conv_for_no_stride):
                cfg = dict(upsample_cfg)
                if cfg.pop('type') != 'deconv':
                    raise NotImplementedError(f'SECONDFPN: upsample_cfg {dict(upsample_cfg)}: only deconv is built')
                layer = nn.ConvTranspose2d(in_channels[i], out_channel, kernel_size=stride, stride=stride, **cfg)
            else:
                stride = int(np.round(1 / stride))
                layer = build_conv_layer(conv_cfg, in_channels=in_channels[i], out_channels=out_channel, kernel_size=stride,
                                         stride=stride)
            deblocks.append(nn.Sequential(layer, build_norm_layer(norm_cfg, out_channel)[1], nn.ReLU(inplace=True)))
        self.deblocks = nn.ModuleList(deblocks)
        self.init_cfg = init_cfg if init_cfg is not None else [dict(type='Kaiming', layer='ConvTranspose2d'),
                                                               dict(type='Constant', layer='NaiveSyncBatchNorm2d', val=1.0)]
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.ConvTranspose2d):      # mmcv kaiming_init: fan_out, relu, normal
                nn.init.kaiming_normal_(m.weight, a=0, mode='fan_out', nonlinearity='relu')
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def forward(self, x):
        assert len(x) == len(self.in_channels)
        ups = [deblock(_lib.as_fp32(x[i])) for i, deblock in enumerate(self.deblocks)]
        return [torch.cat(ups, dim=1) if len(ups) > 1 else ups[0]]
