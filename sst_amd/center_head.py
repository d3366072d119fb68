"""Training and decoding side of CenterHead (csrc/center_head.hip): targets, fused losses, box decoding.

Reference: mmdet3d/models/dense_heads/centerpoint_head.py - get_targets / get_targets_single :385-560 (``center_targets``: one
memset and one launch for the whole batch and every task, instead of a Python loop over every box with a numpy Gaussian, a
host-to-device copy and about twenty scalar-tensor launches each), loss :563-610 (``center_loss``: two launches forward, a zero
fill and two launches backward, no ``.item()``, no permuted copy of the regression maps), get_bboxes / get_task_detections
:612-830, and CenterPointBBoxCoder of mmdet3d/core/bbox/coders/centerpoint_bbox_coders.py (``center_decode``: torch.topk as
``_topk`` composes it, then one launch gathering straight from the NCHW maps).

The head's network (the shared convolution and SeparateHead / DCNSeparateHead, :18-239, the latter over the deformable
convolution of sst_amd/deform_conv.py) is opt-in: CenterHead keeps its configs in ``self.unbuilt`` and ``forward`` raises until
``attach_network()`` builds it.  Circle NMS is not built.  fp32 device tensors only; CPU tensors raise.
"""
import copy
import ctypes
import functools

import torch
from torch import nn

from . import _head_common
from . import _lib
from . import box_ops
from .detectors import HEADS, build_head
from .norm import build_conv_layer, build_norm_layer
from .registry import Registry

BBOX_CODERS = Registry('bbox_coder')  # mmdet.core.bbox.builder.BBOX_CODERS
HEAD_NAMES = ('reg', 'height', 'dim', 'rot', 'vel')
HEAD_CHANNELS = (2, 1, 3, 2, 2)


def build_bbox_coder(cfg):
    return BBOX_CODERS.build(cfg)


_check_f32 = functools.partial(_head_common.check_f32, 'sst_amd.center_head')


def center_targets_box_tile():
    """boxes per workgroup of the targets kernel (a sample with more boxes spans workgroups)"""
    return int(_lib.load().sst_center_targets_box_tile())


def center_loss_tile_cells():
    """heatmap cells per workgroup of the loss forward's first launch"""
    return int(_lib.load().sst_center_loss_tile_cells())


def _task_table(tasks):
    """tasks: the config's list of dicts with ``class_names`` (or plain class counts) -> [(first class, count)]"""
    table, first = [], 0
    for t in tasks:
        n = int(t) if isinstance(t, int) else len(t['class_names'])
        table.append((first, n))
        first += n
    return table


@torch.no_grad()
def center_targets(gt_bboxes_list, gt_labels_list, tasks, train_cfg, norm_bbox=True):
    """-> (heatmaps, anno_boxes, inds, masks): per task a batch-stacked tensor, as CenterHead.get_targets returns them.

    gt_bboxes_list: per sample a [G_i, 7 or 9] fp32 device tensor (x, y, z_bottom, w, l, h, rz [, vx, vy]) or an object with
    ``.tensor``; gt_labels_list: [G_i] integer device tensors.  heatmap [B, C_t, H, W] fp32, anno_box [B, max_objs, 10] fp32,
    ind [B, max_objs] int64, mask [B, max_objs] uint8 are views of one allocation.  The sample offsets come from the shapes:
    nothing is read back."""
    if len(gt_bboxes_list) != len(gt_labels_list) or len(gt_bboxes_list) == 0:
        raise RuntimeError('center_targets: one box set and one label set per sample expected')
    boxes_list = [b.tensor if hasattr(b, 'tensor') else b for b in gt_bboxes_list]
    for b, l in zip(boxes_list, gt_labels_list):
        _lib.require_cuda(b.contiguous(), l.contiguous())
        if b.dtype != torch.float32 or b.dim() != 2 or l.numel() != b.size(0):
            raise RuntimeError(f'center_targets: fp32 boxes [G, 7 or 9] and G labels expected, got {b.dtype} '
                               f'{tuple(b.shape)}, {tuple(l.shape)}')
    dev = boxes_list[0].device
    cols = {b.size(1) for b in boxes_list if b.size(0)}
    if len(cols) > 1 or (cols and not cols <= {7, 9}):
        raise RuntimeError(f'center_targets: boxes of 7 or of 9 columns expected, got {sorted(cols)}')
    cols = cols.pop() if cols else 7
    filled = [b for b in boxes_list if b.size(0)]
    boxes = torch.cat(filled, 0).contiguous() if filled else torch.zeros((0, cols), dtype=torch.float32, device=dev)
    labels = torch.cat([l.reshape(-1).to(device=dev, dtype=torch.long) for l in gt_labels_list]).contiguous()
    off = [0]
    for b in boxes_list:
        off.append(off[-1] + b.size(0))
    box_off = torch.tensor(off, dtype=torch.int32).to(dev, non_blocking=True)

    table = _task_table(tasks)
    batch, n_tasks = len(boxes_list), len(table)
    grid, osf = train_cfg['grid_size'], int(train_cfg['out_size_factor'])
    max_objs = int(train_cfg['max_objs']) * int(train_cfg.get('dense_reg', 1))
    h, w = int(grid[1]) // osf, int(grid[0]) // osf
    lib = _lib.load()
    c_table = _lib.i32array([v for row in table for v in row])
    offsets = (ctypes.c_int64 * (4 * n_tasks))()
    total = lib.sst_center_targets_layout(batch, n_tasks, c_table, int(grid[0]), int(grid[1]), osf, max_objs, offsets)
    if total < 0:
        _lib.check(int(total), 'sst_center_targets_layout')
    out = torch.empty(int(total), dtype=torch.uint8, device=dev)
    _lib.check(lib.sst_center_targets_f32(
        _lib.ptr(boxes), cols, _lib.ptr(labels), _lib.ptr(box_off), boxes.size(0), batch, c_table, n_tasks, int(grid[0]),
        int(grid[1]), _lib.farray(train_cfg['point_cloud_range'][:2]), _lib.farray(train_cfg['voxel_size'][:2]), osf,
        float(train_cfg['gaussian_overlap']), int(train_cfg['min_radius']), max_objs, 1 if norm_bbox else 0, _lib.ptr(out),
        _lib.stream_ptr()), 'sst_center_targets_f32')

    def view(at, dtype, shape):
        n = 1
        for s in shape:
            n *= s
        return out[at:at + n * torch.empty((), dtype=dtype).element_size()].view(dtype).view(shape)

    heatmaps, anno_boxes, inds, masks = [], [], [], []
    for t, (_, count) in enumerate(table):
        heatmaps.append(view(offsets[4 * t], torch.float32, (batch, count, h, w)))
        anno_boxes.append(view(offsets[4 * t + 1], torch.float32, (batch, max_objs, 10)))
        inds.append(view(offsets[4 * t + 2], torch.long, (batch, max_objs)))
        masks.append(view(offsets[4 * t + 3], torch.uint8, (batch, max_objs)))
    return heatmaps, anno_boxes, inds, masks


def _head_arrays(heads):
    ptrs = (ctypes.c_void_p * 5)(*[None if t is None else t.data_ptr() for t in heads])
    chans = _lib.i32array([0 if t is None else t.size(1) for t in heads])
    return ptrs, chans


class _CenterLoss(torch.autograd.Function):

    @staticmethod
    def forward(ctx, logits, reg, height, dim, rot, vel, heatmap, anno_box, ind, mask, cfg):
        heads = (reg, height, dim, rot, vel)
        b, c, h, w = logits.shape
        lib = _lib.load()
        dev = logits.device
        out = torch.empty(2, dtype=torch.float32, device=dev)
        counts = torch.empty(2, dtype=torch.long, device=dev)
        ws = _lib.workspace(lib.sst_center_loss_workspace_bytes(logits.numel()), dev)
        ptrs, chans = _head_arrays(heads)
        _lib.check(lib.sst_center_loss_fwd_f32(
            _lib.ptr(logits), _lib.ptr(heatmap), b, c, h * w, ptrs, chans, _lib.ptr(anno_box), _lib.ptr(ind), _lib.ptr(mask),
            ind.size(1), _lib.farray(cfg['code_weights']), cfg['w_cls'], cfg['w_bbox'], _lib.ptr(out), _lib.ptr(counts),
            _lib.ptr(ws), _lib.stream_ptr()), 'sst_center_loss_fwd_f32')
        ctx.save_for_backward(logits, heatmap, anno_box, ind, mask, counts, *[t for t in heads if t is not None])
        ctx.present = [t is not None for t in heads]
        ctx.cfg = cfg
        ctx.mark_non_differentiable(counts)
        ctx.set_materialize_grads(False)      # a loss nobody differentiates arrives as None: no zero tensor is filled for it
        return out[0], out[1], counts

    @staticmethod
    def backward(ctx, g_hm, g_box, _unused):
        logits, heatmap, anno_box, ind, mask, counts = ctx.saved_tensors[:6]
        it = iter(ctx.saved_tensors[6:])
        heads = [next(it) if p else None for p in ctx.present]
        cfg = ctx.cfg
        b, c, h, w = logits.shape
        g_hm, g_box = (None if g is None else g.to(torch.float32).contiguous() for g in (g_hm, g_box))
        d_logits = torch.empty_like(logits)
        n_code = sum(t.size(1) for t in heads if t is not None)
        d_heads = torch.empty(b * n_code * h * w, dtype=torch.float32, device=logits.device)
        ptrs, chans = _head_arrays(heads)
        _lib.check(_lib.load().sst_center_loss_bwd_f32(
            _lib.ptr(logits), _lib.ptr(heatmap), b, c, h * w, ptrs, chans, _lib.ptr(anno_box), _lib.ptr(ind), _lib.ptr(mask),
            ind.size(1), _lib.farray(cfg['code_weights']), cfg['w_cls'], cfg['w_bbox'], _lib.ptr(g_hm), _lib.ptr(g_box),
            _lib.ptr(counts), _lib.ptr(d_logits), _lib.ptr(d_heads), _lib.stream_ptr()), 'sst_center_loss_bwd_f32')
        grads, at = [], 0
        for t in heads:
            if t is None:
                grads.append(None)
                continue
            grads.append(d_heads[at:at + t.numel()].view(t.shape))
            at += t.numel()
        return (d_logits, *grads, None, None, None, None, None)


def center_loss(heatmap_logits, reg, height, dim, rot, vel, heatmap, anno_box, ind, mask, code_weights, loss_weight_cls=1.0,
                loss_weight_bbox=1.0):
    """-> (loss_heatmap, loss_bbox, counts int64 [2] = (#(heatmap == 1), sum(mask))) of one task.

    heatmap_logits, heatmap [B, C, H, W]; reg [B, 2, H, W], height [B, 1, H, W], dim [B, 3, H, W], rot [B, 2, H, W], vel
    [B, 2, H, W] or None: the head's raw outputs, read where they lie (no concatenated or permuted copy); anno_box
    [B, max_objs, 10], ind int64 [B, max_objs], mask uint8 / bool [B, max_objs]; code_weights: 10 floats.
      loss_heatmap = loss_weight_cls * gaussian_focal_loss(clamp(sigmoid(logits), 1e-4, 1 - 1e-4), heatmap).sum()
                     / max(#(heatmap == 1), 1)
      loss_bbox    = loss_weight_bbox * sum(|pred - anno_box| mask code_weights) / (sum(mask) + 1e-4)
    The logits are not modified.  Both losses carry gradients to the logits and the heads; nothing is read back."""
    heads = (reg, height, dim, rot, vel)
    _check_f32(heatmap_logits, heatmap, anno_box, *heads)
    _lib.require_cuda(ind, mask)
    if heatmap_logits.dim() != 4 or heatmap.shape != heatmap_logits.shape:
        raise RuntimeError(f'center_loss: logits and heatmap of one shape [B, C, H, W] expected, got '
                           f'{tuple(heatmap_logits.shape)} and {tuple(heatmap.shape)}')
    b, _, h, w = heatmap_logits.shape
    for name, t in zip(HEAD_NAMES, heads):
        if t is None and name != 'vel':
            raise RuntimeError(f'center_loss: the {name} head is missing')
        if t is not None and (t.dim() != 4 or t.size(0) != b or tuple(t.shape[2:]) != (h, w)):
            raise RuntimeError(f'center_loss: {name} must be [B, C, H, W] on the heatmap\'s grid, got {tuple(t.shape)}')
    n_code = sum(t.size(1) for t in heads if t is not None)
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    max_objs = ind.size(1) if ind.dim() == 2 else -1
    if (n_code > 10 or tuple(anno_box.shape) != (b, max_objs, 10) or ind.dtype != torch.long or tuple(ind.shape) != (b, max_objs)
            or mask.dtype != torch.uint8 or tuple(mask.shape) != (b, max_objs) or len(code_weights) != 10):
        raise RuntimeError('center_loss: anno_box [B, max_objs, 10], int64 ind and uint8 mask [B, max_objs], ten code weights '
                           'and at most ten head channels expected')
    cfg = dict(code_weights=[float(v) for v in code_weights], w_cls=float(loss_weight_cls), w_bbox=float(loss_weight_bbox))
    return _CenterLoss.apply(heatmap_logits, reg, height, dim, rot, vel, heatmap, anno_box, ind, mask, cfg)


def center_topk(scores, k):
    """CenterPointBBoxCoder._topk (:61-94): per class, then over the classes; torch.topk's tie order.
    scores [B, C, H, W] -> (score [B, K], cell index int64 [B, K], class int32 [B, K])"""
    batch, cat, height, width = scores.size()
    topk_scores, topk_inds = torch.topk(scores.reshape(batch, cat, -1), k)
    topk_inds = topk_inds % (height * width)
    topk_score, topk_ind = torch.topk(topk_scores.view(batch, -1), k)
    topk_clses = (topk_ind / torch.tensor(k, dtype=torch.float)).int()
    topk_inds = topk_inds.view(batch, -1).gather(1, topk_ind)
    return topk_score, topk_inds, topk_clses


@torch.no_grad()
def center_decode(inds, scores, reg, hei, dim, rot_sine, rot_cosine, vel, out_size_factor, voxel_size, pc_range,
                  norm_bbox=False, score_threshold=None, post_center_range=None):
    """-> (boxes [B, K, 9 or 7 without vel], keep bool [B, K]) at the cell indices ``inds`` int64 [B, K] with ``scores`` [B, K].

    reg [B, 2, H, W] or None (then + 0.5), hei [B, 1, H, W], dim [B, 3, H, W] (exp is applied when ``norm_bbox``), rot_sine,
    rot_cosine [B, 1, H, W], vel [B, 2, H, W] or None: read where they lie - a channel slice of a contiguous NCHW tensor is
    fine.  keep = (score > score_threshold) & (post_center_range[:3] <= centre <= post_center_range[3:])."""
    maps = (reg, hei, dim, rot_sine, rot_cosine, vel)
    need = (2, 1, 3, 1, 1, 2)
    _check_f32(scores.contiguous())
    _lib.require_cuda(inds, scores)
    if inds.dtype != torch.long or inds.dim() != 2 or scores.shape != inds.shape:
        raise RuntimeError('center_decode: int64 inds [B, K] and fp32 scores of the same shape expected')
    b, k = inds.shape
    if hei is None or hei.dim() != 4:
        raise RuntimeError('center_decode: hei must be a [B, 1, H, W] map')
    h, w = hei.shape[2:]
    strides = []
    for name, t, c in zip(('reg', 'hei', 'dim', 'rot_sine', 'rot_cosine', 'vel'), maps, need):
        if t is None:
            if name not in ('reg', 'vel'):
                raise RuntimeError(f'center_decode: {name} is missing')
            strides.append(0)
            continue
        if not t.is_cuda or t.dtype != torch.float32:
            raise RuntimeError('sst_amd: fp32 CUDA/HIP tensors expected (no CPU path in this library)')
        if tuple(t.shape) != (b, c, h, w) or t.stride(3) != 1 or t.stride(2) != w or (c > 1 and t.stride(1) != h * w):
            raise RuntimeError(f'center_decode: {name} must be a [B, {c}, H, W] map with dense planes, got {tuple(t.shape)} '
                               f'strides {t.stride()}')
        strides.append(t.stride(0))
    boxes = torch.empty((b, k, 7 if vel is None else 9), dtype=torch.float32, device=inds.device)
    keep = torch.empty((b, k), dtype=torch.uint8, device=inds.device)
    ptrs = (ctypes.c_void_p * 6)(*[None if t is None else t.data_ptr() for t in maps])
    rng = None if post_center_range is None else _lib.farray([float(v) for v in post_center_range])
    _lib.check(_lib.load().sst_center_decode_f32(
        _lib.ptr(inds), _lib.ptr(scores), b, k, w, h * w, ptrs, _lib.i64array(strides), int(out_size_factor),
        _lib.farray(voxel_size[:2]), _lib.farray(pc_range[:2]), 1 if norm_bbox else 0, 0 if score_threshold is None else 1,
        0.0 if score_threshold is None else float(score_threshold), rng, _lib.ptr(boxes), _lib.ptr(keep), _lib.stream_ptr()),
        'sst_center_decode_f32')
    return boxes, keep.bool()


@BBOX_CODERS.register_module()
class CenterPointBBoxCoder(object):
    """core/bbox/coders/centerpoint_bbox_coders.py: the reference's constructor keys and ``decode`` signature"""

    def __init__(self, pc_range, out_size_factor, voxel_size, post_center_range=None, max_num=100, score_threshold=None,
                 code_size=9):
        self.pc_range = pc_range
        self.out_size_factor = out_size_factor
        self.voxel_size = voxel_size
        self.post_center_range = post_center_range
        self.max_num = max_num
        self.score_threshold = score_threshold
        self.code_size = code_size

    def encode(self):
        pass

    def decode_batch(self, heat, rot_sine, rot_cosine, hei, dim, vel, reg=None, norm_bbox=False):
        """-> (boxes [B, K, 9 / 7], scores [B, K], labels int32 [B, K], keep bool [B, K]) without the per-sample compaction"""
        if self.post_center_range is None:
            raise NotImplementedError('Need to reorganize output as a batch, only support post_center_range is not None for now!')
        _check_f32(heat)
        scores, inds, clses = center_topk(heat, self.max_num)
        # `if self.score_threshold:` of the reference (:209): a threshold of None or 0 filters nothing
        thr = self.score_threshold if self.score_threshold else None
        boxes, keep = center_decode(inds.contiguous(), scores.contiguous(), reg, hei, dim, rot_sine, rot_cosine, vel,
                                    self.out_size_factor, self.voxel_size, self.pc_range, norm_bbox=norm_bbox,
                                    score_threshold=thr, post_center_range=self.post_center_range)
        return boxes, scores, clses, keep

    def decode(self, heat, rot_sine, rot_cosine, hei, dim, vel, reg=None, task_id=-1):
        """-> per sample dict(bboxes, scores, labels (float, as the reference's ``clses.float()``)) of the kept boxes"""
        boxes, scores, clses, keep = self.decode_batch(heat, rot_sine, rot_cosine, hei, dim, vel, reg)
        labels = clses.float()
        return [dict(bboxes=boxes[i, keep[i]], scores=scores[i, keep[i]], labels=labels[i, keep[i]])
                for i in range(heat.size(0))]


class ConvModule(nn.Module):
    """mmcv.cnn.ConvModule as the head uses it: ``conv`` -> ``bn`` (the norm's mmcv name) -> ReLU; ``bias='auto'`` gives the
    convolution no bias in front of a norm"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias='auto', conv_cfg=None, norm_cfg=None):
        super().__init__()
        if bias == 'auto':
            bias = norm_cfg is None
        self.conv = build_conv_layer(conv_cfg, in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=bias)
        self.norm_name = None
        if norm_cfg is not None:
            self.norm_name, norm = build_norm_layer(norm_cfg, out_channels)
            self.add_module(self.norm_name, norm)
        self.activate = nn.ReLU(inplace=True)

    def forward(self, x):
        x = self.conv(x)
        if self.norm_name is not None:
            x = getattr(self, self.norm_name)(x)
        return self.activate(x)


@HEADS.register_module()
class SeparateHead(nn.Module):
    """centerpoint_head.py:18-120: per head name a Sequential of (num_conv - 1) ConvModules and a biased convolution.
    Initialisation: torch's Kaiming defaults, the heatmap's last bias ``init_bias`` (parity with mmcv's initialisers is not
    claimed)."""

    def __init__(self, in_channels, heads, head_conv=64, final_kernel=1, init_bias=-2.19, conv_cfg=dict(type='Conv2d'),
                 norm_cfg=dict(type='BN2d'), bias='auto', init_cfg=None, **kwargs):
        assert init_cfg is None, 'To prevent abnormal initialization behavior, init_cfg is not allowed to be set'
        super().__init__()
        self.heads = heads
        self.init_bias = init_bias
        for head in self.heads:
            classes, num_conv = self.heads[head]
            layers, c_in = [], in_channels
            for _ in range(num_conv - 1):
                layers.append(ConvModule(c_in, head_conv, kernel_size=final_kernel, stride=1, padding=final_kernel // 2, bias=bias,
                                         conv_cfg=conv_cfg, norm_cfg=norm_cfg))
                c_in = head_conv
            layers.append(build_conv_layer(conv_cfg, head_conv, classes, kernel_size=final_kernel, stride=1,
                                           padding=final_kernel // 2, bias=True))
            setattr(self, head, nn.Sequential(*layers))
        self.init_weights()

    def init_weights(self):
        for head in self.heads:
            if head == 'heatmap':
                getattr(self, head)[-1].bias.data.fill_(self.init_bias)

    def forward(self, x):
        return {head: getattr(self, head)(x) for head in self.heads}


@HEADS.register_module()
class DCNSeparateHead(nn.Module):
    """centerpoint_head.py:123-239: a deformable convolution in front of the heatmap head and another in front of the
    regression heads (``feature_adapt_cls`` / ``feature_adapt_reg``), ``cls_head`` and the SeparateHead ``task_head``.  As in the
    reference, ``task_head`` is built with SeparateHead's default conv / norm configs.  ``conv_offset`` starts at zero and
    the heatmap's last bias at ``init_bias``; everything else has torch's Kaiming defaults."""

    def __init__(self, in_channels, num_cls, heads, dcn_config, head_conv=64, final_kernel=1, init_bias=-2.19,
                 conv_cfg=dict(type='Conv2d'), norm_cfg=dict(type='BN2d'), bias='auto', init_cfg=None, **kwargs):
        assert init_cfg is None, 'To prevent abnormal initialization behavior, init_cfg is not allowed to be set'
        super().__init__()
        heads = {k: v for k, v in heads.items() if k != 'heatmap'}
        self.feature_adapt_cls = build_conv_layer(dcn_config)
        self.feature_adapt_reg = build_conv_layer(dcn_config)
        self.cls_head = nn.Sequential(
            ConvModule(in_channels, head_conv, kernel_size=3, padding=1, conv_cfg=conv_cfg, bias=bias, norm_cfg=norm_cfg),
            build_conv_layer(conv_cfg, head_conv, num_cls, kernel_size=3, stride=1, padding=1, bias=bool(bias)))
        self.init_bias = init_bias
        self.task_head = SeparateHead(in_channels, heads, head_conv=head_conv, final_kernel=final_kernel, bias=bias)
        self.init_weights()

    def init_weights(self):
        self.cls_head[-1].bias.data.fill_(self.init_bias)

    def forward(self, x):
        center_feat = self.feature_adapt_cls(x)
        reg_feat = self.feature_adapt_reg(x)
        ret = self.task_head(reg_feat)
        ret['heatmap'] = self.cls_head(center_feat)
        return ret


_NETWORK_KEYS = ('in_channels', 'common_heads', 'separate_head', 'share_conv_channel', 'num_heatmap_convs', 'conv_cfg',
                 'norm_cfg', 'bias')


@HEADS.register_module()
class CenterHead(nn.Module):
    """CenterHead (dense_heads/centerpoint_head.py:241-830): targets, losses and box extraction on the kernels of
    csrc/center_head.hip.  The keys of the shared convolution and the task heads (SeparateHead / DCNSeparateHead) are kept in
    ``self.unbuilt`` and ``forward`` raises until ``attach_network()`` builds them (``shared_conv``, ``task_heads``, the
    reference's sub-module names).  ``loss`` and ``get_bboxes`` take the ``preds_dicts`` the forward gives: per task a
    one-element list with a dict of ``heatmap`` / ``reg`` / ``height`` / ``dim`` / ``rot`` / ``vel`` maps."""

    def __init__(self, in_channels=[128], tasks=None, train_cfg=None, test_cfg=None, bbox_coder=None, common_heads=dict(),
                 loss_cls=dict(type='GaussianFocalLoss', reduction='mean'),
                 loss_bbox=dict(type='L1Loss', reduction='none', loss_weight=0.25),
                 separate_head=dict(type='SeparateHead', init_bias=-2.19, final_kernel=3), share_conv_channel=64,
                 num_heatmap_convs=2, conv_cfg=dict(type='Conv2d'), norm_cfg=dict(type='BN2d'), bias='auto', norm_bbox=True,
                 init_cfg=None):
        assert init_cfg is None, 'To prevent abnormal initialization behavior, init_cfg is not allowed to be set'
        super().__init__()
        self.class_names = [t['class_names'] for t in tasks]
        self.num_classes = [len(n) for n in self.class_names]
        self.tasks = list(tasks)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.in_channels = in_channels
        self.norm_bbox = norm_bbox
        self.loss_cfg = dict(loss_cls=dict(loss_cls), loss_bbox=dict(loss_bbox))
        self.bbox_coder = build_bbox_coder(bbox_coder) if bbox_coder is not None else None
        self.fp16_enabled = False
        local = locals()
        self.unbuilt = {k: local[k] for k in _NETWORK_KEYS}
        # what `loss` will run; a config it cannot run is refused there, not here: every shipped config constructs
        self.loss_unbuilt = []
        if loss_cls.get('type') != 'GaussianFocalLoss' or loss_cls.get('reduction', 'mean') != 'mean' \
                or loss_cls.get('alpha', 2.0) != 2.0 or loss_cls.get('gamma', 4.0) != 4.0:
            self.loss_unbuilt.append(f'loss_cls {dict(loss_cls)}: only GaussianFocalLoss (alpha 2, gamma 4, mean) is built')
        if loss_bbox.get('type') != 'L1Loss' or loss_bbox.get('reduction', 'mean') != 'mean':
            self.loss_unbuilt.append(f'loss_bbox {dict(loss_bbox)}: only L1Loss with mean reduction is built')
        self.loss_weight_cls = float(loss_cls.get('loss_weight', 1.0))
        self.loss_weight_bbox = float(loss_bbox.get('loss_weight', 1.0))

    def attach_network(self):
        """Opt in to the head's network: build ``shared_conv`` and ``task_heads`` from ``self.unbuilt`` (:310-327) -> self.
        ``unbuilt`` stays as it is; a head without this call has no parameters and ``forward`` raises."""
        u = self.unbuilt
        in_channels = u['in_channels']
        if isinstance(in_channels, (list, tuple)):
            if len(in_channels) != 1:
                raise NotImplementedError(f'CenterHead.attach_network: in_channels {in_channels}: one feature level is built')
            in_channels = in_channels[0]
        self.shared_conv = ConvModule(in_channels, u['share_conv_channel'], kernel_size=3, padding=1, conv_cfg=u['conv_cfg'],
                                      norm_cfg=u['norm_cfg'], bias=u['bias'])
        self.task_heads = nn.ModuleList()
        for num_cls in self.num_classes:
            heads = copy.deepcopy(dict(u['common_heads']))
            heads.update(dict(heatmap=(num_cls, u['num_heatmap_convs'])))
            cfg = copy.deepcopy(dict(u['separate_head']))
            cfg.update(in_channels=u['share_conv_channel'], heads=heads, num_cls=num_cls)
            self.task_heads.append(build_head(cfg))
        return self

    def forward_single(self, x):
        x = self.shared_conv(_lib.as_fp32(x))
        return [task(x) for task in self.task_heads]

    def forward(self, feats):
        if getattr(self, 'task_heads', None) is None:
            raise NotImplementedError('CenterHead.forward: the shared convolution and the task heads '
                                      f'({self.unbuilt["separate_head"].get("type")}) are not built; sst_amd.CenterHead covers '
                                      'get_targets, loss and get_bboxes on the maps those heads produce')
        if torch.is_tensor(feats):
            feats = [feats]
        # multi_apply(self.forward_single, feats): per task the list over the feature levels
        return tuple(map(list, zip(*[self.forward_single(x) for x in feats])))

    def get_targets(self, gt_bboxes_3d, gt_labels_3d):
        return center_targets(gt_bboxes_3d, gt_labels_3d, self.tasks, self.train_cfg, self.norm_bbox)

    def loss(self, gt_bboxes_3d, gt_labels_3d, preds_dicts, **kwargs):
        if self.loss_unbuilt:
            raise NotImplementedError('; '.join(self.loss_unbuilt))
        heatmaps, anno_boxes, inds, masks = self.get_targets(gt_bboxes_3d, gt_labels_3d)
        code_weights = self.train_cfg.get('code_weights', None)
        loss_dict = dict()
        for task_id, preds_dict in enumerate(preds_dicts):
            p = {k: _lib.as_fp32(v) for k, v in preds_dict[0].items()}   # force_fp32(apply_to=('preds_dicts'))
            loss_heatmap, loss_bbox, _ = center_loss(
                p['heatmap'], p['reg'], p['height'], p['dim'], p['rot'], p.get('vel'), heatmaps[task_id], anno_boxes[task_id],
                inds[task_id], masks[task_id], code_weights, self.loss_weight_cls, self.loss_weight_bbox)
            loss_dict[f'task{task_id}.loss_heatmap'] = loss_heatmap
            loss_dict[f'task{task_id}.loss_bbox'] = loss_bbox
        return loss_dict

    def get_task_detections(self, boxes, scores, labels, keep):
        """get_task_detections :706-830 for one sample of one task, on the decoded [K] candidates and their keep mask"""
        cfg = self.test_cfg
        if cfg['score_threshold'] > 0.0:
            keep = keep & (scores >= cfg['score_threshold'])
        boxes, scores, labels = boxes[keep], scores[keep], labels[keep].long()
        if scores.size(0) == 0:
            return boxes, scores, labels
        bev = box_ops.xywhr2xyxyr(box_ops.lidar_bev(boxes))
        selected = box_ops.nms_gpu(bev, scores, cfg['nms_thr'], pre_maxsize=cfg['pre_max_size'],
                                   post_max_size=cfg['post_max_size'])
        boxes, scores, labels = boxes[selected], scores[selected], labels[selected]
        rng = cfg['post_center_limit_range']
        if rng is not None and len(rng) > 0 and boxes.size(0):
            rng = boxes.new_tensor(rng)
            inside = (boxes[:, :3] >= rng[:3]).all(1) & (boxes[:, :3] <= rng[3:]).all(1)
            boxes, scores, labels = boxes[inside], scores[inside], labels[inside]
        return boxes, scores, labels

    @torch.no_grad()
    def get_bboxes(self, preds_dicts, img_metas, img=None, rescale=False):
        """-> per sample [bboxes (bottom centre; wrapped by img_metas[i]['box_type_3d'] when given), scores, labels int32]"""
        assert self.test_cfg['nms_type'] in ['circle', 'rotate']
        if self.test_cfg['nms_type'] == 'circle':
            raise NotImplementedError('CenterHead.get_bboxes: circle NMS is not built (nms_type=\'rotate\' is)')
        rets = []
        for task_id, preds_dict in enumerate(preds_dicts):
            p = {k: _lib.as_fp32(v) for k, v in preds_dict[0].items()}
            heat = p['heatmap'].sigmoid()
            rot = p['rot']
            boxes, scores, clses, keep = self.bbox_coder.decode_batch(heat, rot[:, 0:1], rot[:, 1:2], p['height'], p['dim'],
                                                                      p.get('vel'), reg=p['reg'], norm_bbox=self.norm_bbox)
            rets.append([self.get_task_detections(boxes[i], scores[i], clses[i], keep[i]) for i in range(heat.size(0))])
        ret_list = []
        for i in range(len(rets[0])):
            bboxes = torch.cat([ret[i][0] for ret in rets])
            bboxes[:, 2] = bboxes[:, 2] - bboxes[:, 5] * 0.5
            box_type = (img_metas[i] or {}).get('box_type_3d') if img_metas is not None else None
            if box_type is not None:
                bboxes = box_type(bboxes, self.bbox_coder.code_size)
            scores = torch.cat([ret[i][1] for ret in rets])
            flag, labels = 0, []
            for j, num_class in enumerate(self.num_classes):
                labels.append((rets[j][i][2] + flag).int())
                flag += num_class
            ret_list.append([bboxes, scores, torch.cat(labels)])
        return ret_list
