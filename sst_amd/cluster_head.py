"""The FSD cluster heads (csrc/cluster_head.hip): SparseClusterHeadV2, FSDV2Head, FSDSeparateHead and BasePointBBoxCoder.

Reference: mmdet3d/models/dense_heads/sparse_cluster_head_v2.py, fsd_v2_head.py, sparse_cluster_head.py and
core/bbox/coders/base_point_bbox_coder.py.  The network (the shared MLP and the per-task attribute MLPs) is built from
``sst_ops.build_mlp``; what the reference runs around it as a Python loop over tasks x samples is three kernels' work here:
``cluster_targets`` (one launch for all tasks and samples instead of, per task and sample, two boolean compactions, a regrouping
of the ground truth, a points-in-boxes launch, an ``.any()`` read-back, an ``encode`` and a masked scatter), ``cluster_loss`` (two
launches forward, one backward for all tasks, no ``nonzero()``, no assert read-back: those are the ``status`` column of
``counts``) and ``cluster_decode`` (one launch per task: decode, padded sigmoid scores, the NMS's box rows).
fp32 device tensors only; CPU, non-fp32 or non-contiguous inputs raise.
"""
import copy
import ctypes
import functools

import torch
from torch import nn

from . import _head_common
from . import _lib
from . import box_ops
from ._head_common import LOSS_COUNTS, LOSS_FINISH, cfg_get as _cfg_get, dist_world as _dist_world
from .center_head import BBOX_CODERS, build_bbox_coder
from .detectors import HEADS, build_head
from .sst_ops import build_mlp

STATUS_BAD_LABEL, STATUS_BAD_FLAG = 1, 2
LOSS_NAMES = ('loss_cls', 'loss_center', 'loss_size', 'loss_rot', 'loss_vel')

_check_f32 = functools.partial(_head_common.check_f32, 'sst_amd.cluster_head')
_check = functools.partial(_head_common.check, 'sst_amd.cluster_head')


def cluster_max_tasks():
    return int(_lib.load().sst_cluster_max_tasks())


def cluster_targets_box_tile():
    """boxes per LDS tile of the targets kernel (a sample with more boxes crosses tiles)"""
    return int(_lib.load().sst_cluster_targets_box_tile())


def cluster_loss_tile_rows():
    """rows per workgroup of the loss forward's first launch"""
    return int(_lib.load().sst_cluster_loss_tile_rows())


def _class_table(tasks, class_names):
    """[(task, class index within the task)] per global class, (-1, 0) for a class of no task; class counts per task"""
    table = [(-1, 0)] * len(class_names)
    for t, task in enumerate(tasks):
        for i, name in enumerate(task['class_names']):
            table[class_names.index(name)] = (t, i)
    return table, [len(t['class_names']) for t in tasks]


def _batch_index(cluster_inds, n):
    """the per-row sample index as (tensor kept alive, pointer, stride in elements): column 1 of [N, k] indices, or a vector"""
    _lib.require_cuda(cluster_inds)
    if cluster_inds.dtype != torch.long:
        cluster_inds = cluster_inds.long()
    if cluster_inds.dim() == 1:
        if cluster_inds.numel() != n:
            raise RuntimeError(f'cluster_targets: {n} batch indices expected, got {cluster_inds.numel()}')
        return cluster_inds, ctypes.c_void_p(cluster_inds.data_ptr()), 1
    if cluster_inds.dim() != 2 or cluster_inds.size(0) != n or cluster_inds.size(1) < 2:
        raise RuntimeError(f'cluster_targets: cluster_inds [N, >= 2] or a batch index [N] expected, got {tuple(cluster_inds.shape)}')
    # an empty tensor may report strides of 0: no row is read then
    return cluster_inds, ctypes.c_void_p(cluster_inds.data_ptr() + 8 * cluster_inds.stride(1)), max(cluster_inds.stride(0), 1)


def _targets_launch(xyz_assign, xyz_base, cluster_inds, gt_bboxes_list, gt_labels_list, table, task_classes, code_size,
                    enlarge_width):
    if len(gt_bboxes_list) != len(gt_labels_list) or len(gt_bboxes_list) == 0:
        raise RuntimeError('cluster_targets: one box set and one label set per sample expected')
    _check_f32(xyz_assign, xyz_base)
    n = xyz_assign.size(0)
    if xyz_assign.dim() != 2 or xyz_assign.size(1) != 3 or xyz_base.shape != xyz_assign.shape:
        raise RuntimeError(f'cluster_targets: xyz [N, 3] expected, got {tuple(xyz_assign.shape)} and {tuple(xyz_base.shape)}')
    dev = xyz_assign.device
    boxes_list = [b.tensor if hasattr(b, 'tensor') else b for b in gt_bboxes_list]
    for b, l in zip(boxes_list, gt_labels_list):
        if b.dtype != torch.float32 or b.dim() != 2 or l.numel() != b.size(0):
            raise RuntimeError(f'cluster_targets: fp32 boxes [G, 7 | 9 | 10] and G labels expected, got {b.dtype} '
                               f'{tuple(b.shape)}, {tuple(l.shape)}')
    cols = {b.size(1) for b in boxes_list if b.size(0)}
    if len(cols) > 1 or (cols and not cols <= {7, 9, 10}):
        raise RuntimeError(f'cluster_targets: boxes of 7, 9 or 10 columns expected, got {sorted(cols)}')
    cols = cols.pop() if cols else (7 if code_size == 8 else 9)
    filled = [b.to(dev) for b in boxes_list if b.size(0)]
    boxes = torch.cat(filled, 0).contiguous() if filled else torch.zeros((0, cols), dtype=torch.float32, device=dev)
    labels = torch.cat([l.reshape(-1).to(device=dev, dtype=torch.long) for l in gt_labels_list]).contiguous()
    off = [0]
    for b in boxes_list:
        off.append(off[-1] + b.size(0))
    box_off = torch.tensor(off, dtype=torch.int32).to(dev, non_blocking=True)
    keep, bptr, bstride = _batch_index(cluster_inds, n)
    n_tasks = len(task_classes)
    lib = _lib.load()
    offsets = (ctypes.c_int64 * (4 * n_tasks))()
    total = lib.sst_cluster_targets_layout(n, n_tasks, code_size, offsets)
    if total < 0:
        _lib.check(int(total), 'sst_cluster_targets_layout')
    out = torch.empty(int(total), dtype=torch.uint8, device=dev)
    _lib.check(lib.sst_cluster_targets_f32(
        _lib.ptr(xyz_assign), _lib.ptr(xyz_base), n, bptr, bstride, len(boxes_list), _lib.ptr(boxes), cols, _lib.ptr(labels),
        _lib.ptr(box_off), boxes.size(0), _lib.i32array([v for row in table for v in row]), len(table),
        _lib.i32array(task_classes), n_tasks, code_size, 0 if enlarge_width is None else 1,
        0.0 if enlarge_width is None else float(enlarge_width), _lib.ptr(out), _lib.stream_ptr()), 'sst_cluster_targets_f32')
    del keep

    def view(at, dtype, shape):
        count = 1
        for s in shape:
            count *= s
        return out[at:at + count * torch.empty((), dtype=dtype).element_size()].view(dtype).view(shape)

    res = []
    for t in range(n_tasks):
        res.append((view(offsets[4 * t], torch.long, (n,)), view(offsets[4 * t + 3], torch.int32, (n,)),
                    view(offsets[4 * t + 1], torch.float32, (n, code_size)), view(offsets[4 * t + 2], torch.float32, (n, code_size))))
    return res, labels


@torch.no_grad()
def cluster_targets(xyz, cluster_inds, gt_bboxes_list, gt_labels_list, tasks, class_names, code_size=8, enlarge_width=None,
                    xyz_base=None):
    """-> per task (labels int64 [N], assigned int32 [N], bbox_targets [N, code_size], bbox_weights [N, code_size]): views of one
    allocation, written by ONE launch for all tasks and samples.

    xyz [N, 3]: the points tested for membership; xyz_base: the points the regression is relative to (default: xyz; they differ
    under FSDV2Head's centroid_assign).  cluster_inds: int64 [N, >= 2] whose column 1 is the sample of the row (read in place,
    rows of different samples may interleave) or the sample vector [N].  gt_bboxes_list: per sample [G_i, 7 | 9 | 10] fp32
    tensors or objects with ``.tensor``; gt_labels_list: GLOBAL class indices (boxes with a label < 0 or of no task are skipped).
    tasks: the config's list of dict(class_names=[...]); class_names: the global class list.  Per task the assigned box is the
    hit with the smallest (class index within the task, box index): the first hit of the reference's regrouped list.  Nothing is
    read back."""
    if isinstance(enlarge_width, dict):
        raise NotImplementedError('cluster_targets: the dict form of enlarge_width (scaled_box) is not built')
    table, task_classes = _class_table(tasks, class_names)
    res, _ = _targets_launch(xyz, xyz if xyz_base is None else xyz_base, cluster_inds, gt_bboxes_list, gt_labels_list, table,
                             task_classes, int(code_size), enlarge_width)
    return res


def _task_array(logits, regs, labels, tgts, wts, d_logits=None, d_regs=None):
    arr = (_lib.ClusterLossTask * len(logits))()
    for t in range(len(logits)):
        arr[t].logits, arr[t].reg_preds, arr[t].labels = logits[t].data_ptr(), regs[t].data_ptr(), labels[t].data_ptr()
        arr[t].bbox_targets, arr[t].bbox_weights = tgts[t].data_ptr(), wts[t].data_ptr()
        arr[t].d_logits = d_logits[t].data_ptr() if d_logits is not None else None
        arr[t].d_reg_preds = d_regs[t].data_ptr() if d_regs is not None else None
        arr[t].classes = logits[t].size(1)
    return arr


class _ClusterLoss(torch.autograd.Function):

    @staticmethod
    def forward(ctx, cfg, n_tasks, *tensors):
        logits, regs, labels, tgts, wts = (tensors[k * n_tasks:(k + 1) * n_tasks] for k in range(5))
        n, code = regs[0].shape
        lib = _lib.load()
        dev = regs[0].device
        out = torch.empty((n_tasks, 5), dtype=torch.float32, device=dev)
        counts = torch.empty((n_tasks, 4), dtype=torch.float64, device=dev)
        ws = _lib.workspace(lib.sst_cluster_loss_workspace_bytes(n, n_tasks), dev)
        arr = _task_array(logits, regs, labels, tgts, wts)
        cw = None if cfg['code_weight'] is None else _lib.farray(cfg['code_weight'])
        lw = _lib.farray(cfg['loss_weights'])

        def launch(phases):
            _lib.check(lib.sst_cluster_loss_fwd_f32(arr, n_tasks, n, code, cfg['gamma'], cfg['alpha'], cw, lw, _lib.farray(cfg['beta']), phases,
                                                    _lib.ptr(out), _lib.ptr(counts), _lib.ptr(ws), _lib.stream_ptr()),
                       'sst_cluster_loss_fwd_f32')

        world = _dist_world()
        sync = [k for k, on in ((2, cfg['sync_cls']), (3, cfg['sync_reg'])) if on]
        if world > 1 and sync:
            # reduce_mean of the averaging factors, on the device: counts is written by the first call and read by the second
            launch(LOSS_COUNTS)
            avg = counts[:, sync].contiguous()
            torch.distributed.all_reduce(avg.div_(world))
            counts[:, sync] = avg
            launch(LOSS_FINISH)
        else:
            launch(LOSS_COUNTS | LOSS_FINISH)
        ctx.save_for_backward(counts, *tensors)
        ctx.cfg, ctx.n_tasks = cfg, n_tasks
        ctx.mark_non_differentiable(counts)
        ctx.set_materialize_grads(False)      # a loss nobody differentiates arrives as None: no zero tensor is filled for it
        # every loss is an output of its own: summing them costs autograd nothing per loss (a [T, 5] output indexed by the caller
        # would bring a zero fill and a scatter per loss into the backward)
        return (counts, *[out[t, k] for t in range(n_tasks) for k in range(5)])

    @staticmethod
    def backward(ctx, _unused, *g_losses):
        counts = ctx.saved_tensors[0]
        tensors = ctx.saved_tensors[1:]
        cfg, n_tasks = ctx.cfg, ctx.n_tasks
        logits, regs, labels, tgts, wts = (tensors[k * n_tasks:(k + 1) * n_tasks] for k in range(5))
        n, code = regs[0].shape
        zero = regs[0].new_zeros(())
        g = torch.stack([zero if x is None else x.reshape(()).to(torch.float32) for x in g_losses])
        d_logits = [torch.empty_like(t) for t in logits]
        d_regs = [torch.empty_like(t) for t in regs]
        arr = _task_array(logits, regs, labels, tgts, wts, d_logits, d_regs)
        cw = None if cfg['code_weight'] is None else _lib.farray(cfg['code_weight'])
        _lib.check(_lib.load().sst_cluster_loss_bwd_f32(arr, n_tasks, n, code, cfg['gamma'], cfg['alpha'], cw,
                                                        _lib.farray(cfg['loss_weights']), _lib.farray(cfg['beta']), _lib.ptr(g),
                                                        _lib.ptr(counts),
                                                        _lib.stream_ptr()), 'sst_cluster_loss_bwd_f32')
        return (None, None, *d_logits, *d_regs, *([None] * (3 * n_tasks)))


def cluster_loss(cls_logits, reg_preds, labels, bbox_targets, bbox_weights, *, gamma=2.0, alpha=0.25,
                 loss_weights=(1.0, 1.0, 1.0, 1.0, 1.0), code_weight=None, smooth_l1_beta=None, sync_cls_avg_factor=False, sync_reg_avg_factor=False):
    """-> (losses: per task the five 0-dim tensors (loss_cls, loss_center, loss_size, loss_rot, loss_vel), counts float64
    [T, 4] = (num_pos, status, cls_avg, reg_avg)).

    Per task: cls_logits [N, C_t], reg_preds / bbox_targets / bbox_weights [N, code] (code 8 or 10), labels int64 [N] (C_t =
    background).  loss_cls = w sum(focal) / cls_avg, loss_center / size / rot = w sum(|pred - target| weight code_weight) /
    reg_avg over columns 0-2 / 3-5 / 6-7 of the positive rows, loss_vel = w sum(columns 8-9) / (2 num_pos); cls_avg = N and
    reg_avg = num_pos, each averaged over the processes of an initialised process group when its ``sync_*`` flag is set
    (reduce_mean, on the device).  smooth_l1_beta: five floats in the order of the loss weights (the first is not used); a
    regression loss with beta > 0 is mmdet's SmoothL1Loss, otherwise its L1Loss.  status: STATUS_BAD_LABEL | STATUS_BAD_FLAG.  The losses carry gradients to every task's
    logits and predictions (one launch); nothing is read back to the host."""
    n_tasks = len(cls_logits)
    if not (n_tasks == len(reg_preds) == len(labels) == len(bbox_targets) == len(bbox_weights)) or n_tasks < 1:
        raise RuntimeError('cluster_loss: per task one tensor of each kind expected')
    if n_tasks > 8:
        raise RuntimeError(f'cluster_loss: at most 8 tasks, got {n_tasks}')
    _check_f32(*cls_logits, *reg_preds, *bbox_targets, *bbox_weights)
    if reg_preds[0].dim() != 2 or reg_preds[0].size(1) not in (8, 10):
        raise RuntimeError(f'cluster_loss: reg_preds [N, 8 | 10] expected, got {tuple(reg_preds[0].shape)}')
    n, code = reg_preds[0].shape
    for t in range(n_tasks):
        if cls_logits[t].dim() != 2 or cls_logits[t].size(0) != n or not 1 <= cls_logits[t].size(1) <= 32:
            raise RuntimeError(f'cluster_loss: logits [N, 1 <= C <= 32] expected, got {tuple(cls_logits[t].shape)}')
        _check(reg_preds[t], torch.float32, (n, code), 'reg_preds')
        _check(bbox_targets[t], torch.float32, (n, code), 'bbox_targets')
        _check(bbox_weights[t], torch.float32, (n, code), 'bbox_weights')
        _check(labels[t], torch.long, (n,), 'labels')
    if code_weight is not None and len(code_weight) != code:
        raise RuntimeError(f'cluster_loss: code_weight needs {code} entries, got {len(code_weight)}')
    if len(loss_weights) != 5:
        raise RuntimeError('cluster_loss: five loss weights (cls, center, size, rot, vel) expected')
    if n == 0:
        # the reference divides 0 by an averaging factor of 0 here; an empty batch gives zeros that still reach the graph
        zero = sum(t.sum() for t in cls_logits) * 0 + sum(t.sum() for t in reg_preds) * 0
        return [(zero,) * 5 for _ in range(n_tasks)], torch.zeros((n_tasks, 4), dtype=torch.float64, device=reg_preds[0].device)
    cfg = dict(gamma=float(gamma), alpha=float(alpha), loss_weights=[float(v) for v in loss_weights],
               code_weight=None if code_weight is None else [float(v) for v in code_weight],
               beta=[0.0] * 5 if smooth_l1_beta is None else [float(v) for v in smooth_l1_beta], sync_cls=bool(sync_cls_avg_factor), sync_reg=bool(sync_reg_avg_factor))
    counts, *flat = _ClusterLoss.apply(cfg, n_tasks, *cls_logits, *reg_preds, *labels, *bbox_targets, *bbox_weights)
    return [tuple(flat[5 * t:5 * t + 5]) for t in range(n_tasks)], counts


@torch.no_grad()
def cluster_encode(bboxes, base_points, code_size=8):
    """BasePointBBoxCoder.encode: bboxes [P, 7 | 9 | 10], base_points [P, 3] -> [P, code_size]"""
    _check_f32(bboxes, base_points)
    if bboxes.dim() != 2 or bboxes.size(1) not in (7, 9, 10) or tuple(base_points.shape) != (bboxes.size(0), 3):
        raise RuntimeError(f'cluster_encode: bboxes [P, 7 | 9 | 10] and base_points [P, 3] expected, got {tuple(bboxes.shape)}, '
                           f'{tuple(base_points.shape)}')
    out = torch.empty((bboxes.size(0), code_size), dtype=torch.float32, device=bboxes.device)
    _lib.check(_lib.load().sst_cluster_encode_f32(_lib.ptr(bboxes), bboxes.size(1), _lib.ptr(base_points), bboxes.size(0),
                                                  int(code_size), _lib.ptr(out), _lib.stream_ptr()), 'sst_cluster_encode_f32')
    return out


@torch.no_grad()
def cluster_decode(reg_preds, base_points, cls_logits=None, with_bev=True):
    """-> (boxes [N, 7 | 9], scores [N, C + 1] or None, bev [N, 5] or None) of one task in one launch.

    boxes = BasePointBBoxCoder.decode(reg_preds [N, 8 | 10], base_points [N, 3]); scores = sigmoid(cls_logits [N, C]) with the
    zero padding column box3d_multiclass_nms expects; bev = (x - w / 2, y - l / 2, x + w / 2, y + l / 2, yaw): what
    xywhr2xyxyr(boxes.bev) gives."""
    _check_f32(reg_preds, base_points, cls_logits)
    if reg_preds.dim() != 2 or reg_preds.size(1) not in (8, 10) or tuple(base_points.shape) != (reg_preds.size(0), 3):
        raise RuntimeError(f'cluster_decode: reg_preds [N, 8 | 10] and base_points [N, 3] expected, got {tuple(reg_preds.shape)}, '
                           f'{tuple(base_points.shape)}')
    n, code = reg_preds.shape
    dev = reg_preds.device
    c = 0
    scores = None
    if cls_logits is not None:
        if cls_logits.dim() != 2 or cls_logits.size(0) != n or cls_logits.size(1) < 1:
            raise RuntimeError(f'cluster_decode: cls_logits [N, C >= 1] expected, got {tuple(cls_logits.shape)}')
        c = cls_logits.size(1)
        scores = torch.empty((n, c + 1), dtype=torch.float32, device=dev)
    boxes = torch.empty((n, code - 1), dtype=torch.float32, device=dev)
    bev = torch.empty((n, 5), dtype=torch.float32, device=dev) if with_bev else None
    _lib.check(_lib.load().sst_cluster_decode_f32(_lib.ptr(reg_preds), _lib.ptr(base_points), _lib.ptr(cls_logits), n, code, c,
                                                  _lib.ptr(boxes), _lib.ptr(scores), _lib.ptr(bev), _lib.stream_ptr()),
               'sst_cluster_decode_f32')
    return boxes, scores, bev


@BBOX_CODERS.register_module()
class BasePointBBoxCoder(object):
    """core/bbox/coders/base_point_bbox_coder.py: the reference's constructor keys; encode / decode run on the kernels"""

    def __init__(self, post_center_range=None, score_thresh=0.1, num_classes=3, max_num=500, code_size=8):
        self.post_center_range = post_center_range
        self.code_size = code_size
        self.EPS = 1e-6
        self.score_thresh = score_thresh
        self.num_classes = num_classes
        self.max_num = max_num

    def encode(self, bboxes, base_points):
        assert bboxes.size(1) in (7, 9, 10), f'bboxes shape: {bboxes.shape}'
        assert bboxes.size(0) == base_points.size(0)
        if bboxes.size(1) in (9, 10):
            assert self.code_size == 10
        return cluster_encode(bboxes, base_points, 8 if bboxes.size(1) == 7 else 10)

    def decode(self, reg_preds, base_points, detach_yaw=False):
        if detach_yaw:
            raise NotImplementedError('BasePointBBoxCoder.decode: detach_yaw=True is the corner loss\'s differentiable decode, '
                                      'which is not built')
        assert reg_preds.size(1) in (8, 10)
        assert reg_preds.size(1) == self.code_size
        return cluster_decode(reg_preds, base_points, with_bev=False)[0]


@HEADS.register_module()
class FSDSeparateHead(nn.Module):
    """sparse_cluster_head_v2.py:17-41: one MLP per attribute, ``attrs[name] = (out_dim, num_layer, hidden_dim)``"""

    def __init__(self, in_channels, attrs, norm_cfg=dict(type='LN'), act='relu', init_cfg=None):
        super().__init__()
        self.attrs = attrs
        for attr_name in self.attrs:
            out_dim, num_layer, hidden_dim = self.attrs[attr_name]
            mlp = build_mlp(in_channels, [hidden_dim, ] * num_layer + [out_dim, ], norm_cfg, is_head=True, act=act)
            self.__setattr__(attr_name, mlp)

    def forward(self, x):
        return {attr_name: self.__getattr__(attr_name)(x) for attr_name in self.attrs}


def _check_l1(name, cfg):
    """-> (loss weight, SmoothL1Loss beta or 0 for L1Loss) of a regression loss config"""
    if cfg is None:
        return 0.0, 0.0
    if cfg.get('type') not in ('L1Loss', 'SmoothL1Loss') or cfg.get('reduction', 'mean') != 'mean':
        raise NotImplementedError(f'{name} {dict(cfg)}: only L1Loss and SmoothL1Loss with mean reduction are built')
    beta = float(cfg.get('beta', 1.0)) if cfg['type'] == 'SmoothL1Loss' else 0.0
    if cfg['type'] == 'SmoothL1Loss' and not beta > 0:
        raise NotImplementedError(f'{name} {dict(cfg)}: SmoothL1Loss needs beta > 0')
    return float(cfg.get('loss_weight', 1.0)), beta


class _ClusterHead(nn.Module):
    """what SparseClusterHeadV2 and FSDV2Head share: the constructor (sparse_cluster_head.py:20-98 + the task heads), forward,
    the fused loss, get_targets and get_bboxes"""

    def __init__(self, num_classes, bbox_coder, loss_cls, loss_center, loss_size, loss_rot, in_channel, shared_mlp_dims, tasks,
                 class_names, common_attrs, num_cls_layer, cls_hidden_dim, separate_head, cls_mlp=None, reg_mlp=None,
                 iou_mlp=None, train_cfg=None, test_cfg=None, norm_cfg=dict(type='LN'), loss_iou=None, act='relu',
                 corner_loss_cfg=None, enlarge_width=None, as_rpn=False, init_cfg=None, shared_dropout=0, loss_vel=None):
        super().__init__()
        kind = type(self).__name__
        if loss_iou is not None:
            raise NotImplementedError(f'{kind}: loss_iou is not built')
        if iou_mlp is not None:
            raise NotImplementedError(f'{kind}: iou_mlp is not built')
        if corner_loss_cfg is not None:
            raise NotImplementedError(f'{kind}: corner_loss_cfg is not built')
        if isinstance(enlarge_width, dict):
            raise NotImplementedError(f'{kind}: the dict form of enlarge_width (scaled_box) is not built')
        if loss_cls.get('type') != 'FocalLoss' or not loss_cls.get('use_sigmoid', False) \
                or loss_cls.get('reduction', 'mean') != 'mean':
            raise NotImplementedError(f'{kind}: loss_cls {dict(loss_cls)}: only the sigmoid FocalLoss with mean reduction is built')
        reg = [_check_l1('loss_center', loss_center), _check_l1('loss_size', loss_size), _check_l1('loss_rot', loss_rot),
               _check_l1('loss_vel', loss_vel)]
        self.loss_weights = [float(loss_cls.get('loss_weight', 1.0))] + [w for w, _ in reg]
        self.smooth_l1_beta = [0.0] + [b for _, b in reg]
        self.gamma, self.alpha = float(loss_cls.get('gamma', 2.0)), float(loss_cls.get('alpha', 0.25))
        self.with_vel = loss_vel is not None
        self.print_info = {}
        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.box_code_size = self.bbox_coder.code_size
        self.num_classes = num_classes
        self.enlarge_width = enlarge_width
        self.sync_reg_avg_factor = False if train_cfg is None else _cfg_get(train_cfg, 'sync_reg_avg_factor', True)
        self.sync_cls_avg_factor = False if train_cfg is None else _cfg_get(train_cfg, 'sync_cls_avg_factor', False)
        self.as_rpn = as_rpn
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.cfg = test_cfg if test_cfg is not None else train_cfg
        self.fp16_enabled = False

        # the module tree - and the order of the RNG draws - of the reference: shared_mlp, conv_cls, conv_reg, then the task heads
        self.shared_mlp = None
        if len(shared_mlp_dims) > 0:
            self.shared_mlp = build_mlp(in_channel, shared_mlp_dims, norm_cfg, act=act, dropout=shared_dropout)
        end_channel = shared_mlp_dims[-1] if len(shared_mlp_dims) > 0 else in_channel
        # the V1 head's conv_cls / conv_reg are constructed and dropped by the reference (`self.conv_cls = None`)
        if cls_mlp is not None:
            build_mlp(end_channel, cls_mlp + [num_classes, ], norm_cfg, True, act=act)
        else:
            nn.Linear(end_channel, num_classes)
        if reg_mlp is not None:
            build_mlp(end_channel, reg_mlp + [self.box_code_size, ], norm_cfg, True, act=act)
        else:
            nn.Linear(end_channel, self.box_code_size)
        self.conv_cls = None
        self.conv_reg = None

        self.tasks = tasks
        self.task_heads = nn.ModuleList()
        separate_head = dict(separate_head)
        for t in tasks:
            attrs = copy.deepcopy(common_attrs)
            attrs.update(dict(score=(len(t['class_names']), num_cls_layer, cls_hidden_dim), ))
            separate_head.update(in_channels=end_channel, attrs=attrs)
            self.task_heads.append(build_head(separate_head))
        self.class_names = class_names
        all_names = []
        for t in tasks:
            all_names += t['class_names']
        self._check_names(all_names, class_names)
        if len(tasks) > 8:
            raise NotImplementedError(f'{kind}: at most 8 tasks, got {len(tasks)}')

    def forward(self, feats, pts_xyz=None, pts_inds=None):
        if self.shared_mlp is not None:
            feats = self.shared_mlp(feats)
        cls_logit_list, reg_pred_list = [], []
        for h in self.task_heads:
            ret = h(feats)
            parts = [ret['center'], ret['dim'], ret['rot']] + ([ret['vel']] if 'vel' in ret else [])
            cls_logit_list.append(ret['score'])
            reg_pred_list.append(torch.cat(parts, dim=-1))
        return dict(cls_logits=cls_logit_list, reg_preds=reg_pred_list)

    def _refuse_train_cfg(self):
        for key in ('assign_by_dist', 'max_assign_dist'):
            if _cfg_get(self.train_cfg, key, None):
                raise NotImplementedError(f'{type(self).__name__}: train_cfg[\'{key}\'] is not built')

    def _assign_xyz(self, xyz, aux_xyz):
        return xyz

    def get_targets(self, num_task_classes, cluster_xyz, batch_idx, gt_bboxes_3d, gt_labels_3d, reg_preds=None, aux_xyz=None):
        """the reference's per-task call: gt_labels_3d are class indices WITHIN the task, as modify_gt_for_single_task leaves
        them; the assigned box is the first hit in the order given.  -> (labels, label_weights, bbox_targets, bbox_weights,
        iou_labels = None)"""
        self._refuse_train_cfg()
        xyz = _lib.as_fp32(cluster_xyz).contiguous()
        table = [(0, 0)] * int(num_task_classes)        # one class for the ordering: the first hit in index order
        res, gt_labels = _targets_launch(self._assign_xyz(xyz, aux_xyz), xyz, batch_idx, gt_bboxes_3d, gt_labels_3d, table, [1],
                                         self.box_code_size, self.enlarge_width)
        _, assigned, bbox_targets, bbox_weights = res[0]
        labels = gt_labels.new_full((xyz.size(0),), int(num_task_classes))
        if gt_labels.numel():
            labels = torch.where(assigned >= 0, gt_labels[assigned.clamp(min=0).long()], labels)
        return labels, xyz.new_ones(xyz.size(0)), bbox_targets, bbox_weights, None

    def loss(self, cls_logits, reg_preds, cluster_xyz, cluster_inds, gt_bboxes_3d, gt_labels_3d, img_metas=None,
             iou_logits=None, gt_bboxes_ignore=None, aux_xyz=None):
        assert isinstance(cls_logits, list) and isinstance(reg_preds, list)
        assert len(cls_logits) == len(reg_preds) == len(self.tasks)
        self._refuse_train_cfg()
        if iou_logits is not None:
            raise NotImplementedError(f'{type(self).__name__}: loss_iou / iou_logits is not built')
        cls_logits = [_lib.as_fp32(t).contiguous() for t in cls_logits]       # force_fp32
        reg_preds = [_lib.as_fp32(t).contiguous() for t in reg_preds]
        xyz = _lib.as_fp32(cluster_xyz).contiguous()
        tg = cluster_targets(self._assign_xyz(xyz, aux_xyz), cluster_inds, gt_bboxes_3d, gt_labels_3d, self.tasks,
                             self.class_names, self.box_code_size, self.enlarge_width, xyz_base=xyz)
        code_weight = _cfg_get(self.train_cfg, 'code_weight', None)
        losses, counts = cluster_loss(cls_logits, reg_preds, [t[0] for t in tg], [t[2] for t in tg], [t[3] for t in tg],
                                      gamma=self.gamma, alpha=self.alpha, loss_weights=self.loss_weights,
                                      code_weight=list(code_weight) if code_weight else None, smooth_l1_beta=self.smooth_l1_beta,
                                      sync_cls_avg_factor=self.sync_cls_avg_factor, sync_reg_avg_factor=self.sync_reg_avg_factor)
        self.last_counts = counts
        out = {}
        for t in range(len(self.tasks)):
            for k, name in enumerate(LOSS_NAMES[:5 if self.with_vel else 4]):
                out[f'{name}.task{t}'] = losses[t][k]
        return out

    def _box_cfg(self):
        if self.as_rpn:
            return _cfg_get(self.train_cfg if self.training else self.test_cfg, 'rpn')
        return self.test_cfg

    @torch.no_grad()
    def get_bboxes(self, cls_logits, reg_preds, cluster_xyz, cluster_inds, input_metas, iou_logits=None, rescale=False):
        """-> per sample (boxes, scores, labels as global class indices); boxes are wrapped by input_metas[i]['box_type_3d'] when
        given.  Per task one decode launch; per (task, sample) nms_pre (torch.topk) and box3d_multiclass_nms."""
        assert isinstance(cls_logits, list) and isinstance(reg_preds, list)
        assert len(cls_logits) == len(reg_preds) == len(self.tasks)
        if iou_logits is not None:
            raise NotImplementedError(f'{type(self).__name__}: iou_logits (loss_iou) is not built')
        cfg = self._box_cfg()
        batch_inds = cluster_inds if cluster_inds.dim() == 1 else cluster_inds[:, 1]
        batch_size = len(input_metas)
        xyz = _lib.as_fp32(cluster_xyz).contiguous()
        rows = [None] if batch_size == 1 else [(batch_inds == i).nonzero(as_tuple=False).reshape(-1) for i in range(batch_size)]
        per_task = []
        for t, task in enumerate(self.tasks):
            logits, reg = _lib.as_fp32(cls_logits[t]).contiguous(), _lib.as_fp32(reg_preds[t]).contiguous()
            assert logits.size(0) == reg.size(0) == xyz.size(0)
            assert logits.size(1) == len(task['class_names']) and reg.size(1) == self.box_code_size
            boxes, scores, bev = cluster_decode(reg, xyz, logits)
            to_global = torch.tensor([self.class_names.index(name) for name in task['class_names']], dtype=torch.long)
            to_global = to_global.to(xyz.device, non_blocking=True)
            per_task.append([self._get_bboxes_single(cfg, boxes, scores, bev, sel, to_global) for sel in rows])
        out = []
        all_task_max_num = self._all_task_max_num()
        for i in range(batch_size):
            boxes = torch.cat([r[i][0] for r in per_task])
            scores = torch.cat([r[i][1] for r in per_task])
            labels = torch.cat([r[i][2] for r in per_task])
            if all_task_max_num is not None and scores.size(0) > all_task_max_num:
                top = scores.topk(all_task_max_num)[1]
                boxes, scores, labels = boxes[top], scores[top], labels[top]
            box_type = (input_metas[i] or {}).get('box_type_3d')
            if box_type is not None:
                boxes = box_type(boxes, boxes.size(1))
            out.append((boxes, scores, labels))
        return out

    def _all_task_max_num(self):
        return None

    def _get_bboxes_single(self, cfg, boxes, scores, bev, sel, to_global):
        if sel is not None:
            boxes, scores, bev = boxes[sel], scores[sel], bev[sel]
        if scores.size(0) == 0:
            return boxes.new_zeros((0, boxes.size(1))), boxes.new_zeros(0), boxes.new_zeros(0, dtype=torch.long)
        nms_pre = _cfg_get(cfg, 'nms_pre', -1)
        if nms_pre > 0 and scores.size(0) > nms_pre:
            max_scores, _ = scores[:, :-1].max(dim=1)
            _, topk_inds = max_scores.topk(nms_pre)
            boxes, scores, bev = boxes[topk_inds], scores[topk_inds], bev[topk_inds]
        out_boxes, out_scores, out_labels = box_ops.box3d_multiclass_nms(boxes, bev.contiguous(), scores,
                                                                         _cfg_get(cfg, 'score_thr', 0), _cfg_get(cfg, 'max_num'),
                                                                         cfg)
        return out_boxes, out_scores, to_global[out_labels]


@HEADS.register_module()
class SparseClusterHeadV2(_ClusterHead):
    """dense_heads/sparse_cluster_head_v2.py:44-576 with the reference's constructor signature and module tree; ``loss`` runs
    one targets launch and the fused losses of all tasks, ``get_bboxes`` the decode kernel and the grouped NMS."""

    def _check_names(self, all_names, class_names):
        assert all_names == class_names

    def loss(self, cls_logits, reg_preds, cluster_xyz, cluster_inds, gt_bboxes_3d, gt_labels_3d, img_metas=None,
             iou_logits=None, gt_bboxes_ignore=None):
        return super().loss(cls_logits, reg_preds, cluster_xyz, cluster_inds, gt_bboxes_3d, gt_labels_3d, img_metas, iou_logits,
                            gt_bboxes_ignore)

    def get_targets(self, num_task_classes, cluster_xyz, batch_idx, gt_bboxes_3d, gt_labels_3d, reg_preds=None):
        return super().get_targets(num_task_classes, cluster_xyz, batch_idx, gt_bboxes_3d, gt_labels_3d, reg_preds)


@HEADS.register_module()
class FSDV2Head(_ClusterHead):
    """dense_heads/fsd_v2_head.py:17-591: the same head over virtual voxels; the task's class order may differ from the global
    one, ``train_cfg['centroid_assign']`` tests ``aux_xyz`` for membership while regressing from ``voxel_xyz``, and
    ``test_cfg['all_task_max_num']`` caps the boxes of a sample."""

    def _check_names(self, all_names, class_names):
        assert len(all_names) == len(class_names)

    def _assign_xyz(self, xyz, aux_xyz):
        if _cfg_get(self.train_cfg, 'centroid_assign', False):
            assert aux_xyz is not None
            return _lib.as_fp32(aux_xyz).contiguous()
        return xyz

    def _all_task_max_num(self):
        return _cfg_get(self.test_cfg, 'all_task_max_num', None)
