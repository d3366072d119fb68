"""Training side of VoteSegHead: the point targets of a batch and the fused decode / vote losses (csrc/seg_loss.hip).

Reference: mmdet3d/models/decode_heads/segmentation_head.py - get_targets :212-249, get_point_labels :252-258,
get_vote_target :260-272, encode_vote_targets :274-275 (``seg_point_targets``: one launch for the whole batch instead of a Python
loop over the samples with a points-in-boxes launch and several boolean-index compactions each) and losses :106-173
(``seg_vote_loss``: two launches forward, one backward, no host read - the reference reads ``seg_label.max()``,
``valid_label.max()``, ``.min()`` and ``num_valid > 0`` back; here those asserts are the ``status`` word of ``counts``).
fp32 device tensors only; CPU, non-contiguous or non-fp32 inputs raise.
"""
import functools

import torch

from . import _head_common
from . import _lib
from ._head_common import offsets as _offsets

SIGMOID_FOCAL, SOFTMAX_CE = 0, 1
STATUS_BAD_LABEL, STATUS_MASKED_NO_CLASS = 1, 2

_check_f32 = functools.partial(_head_common.check_f32, 'sst_amd.seg_loss')
_check = functools.partial(_head_common.check, 'sst_amd.seg_loss')


def seg_targets_box_tile():
    """boxes per LDS tile of the targets kernel (a sample with more boxes crosses tiles)"""
    return int(_lib.load().sst_seg_targets_box_tile())


def seg_loss_tile_rows():
    """points per workgroup of the loss forward's first launch"""
    return int(_lib.load().sst_seg_loss_tile_rows())


def _targets_launch(points, pt_off, batch, boxes, box_labels, box_off, extra_width, bg_label, centers):
    n, g = points.size(0), boxes.size(0)
    dev = points.device
    inbox = torch.empty(n, dtype=torch.int32, device=dev)
    labels = torch.empty(n, dtype=torch.long, device=dev)
    targets = torch.empty((n, 3), dtype=torch.float32, device=dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    if n > 0:
        _lib.check(_lib.load().sst_seg_targets_f32(
            _lib.ptr(points), points.stride(0), n, _lib.ptr(pt_off), batch, _lib.ptr(boxes), _lib.ptr(box_labels),
            _lib.ptr(box_off), g, 0 if extra_width is None else 1, 0.0 if extra_width is None else float(extra_width),
            int(bg_label), _lib.ptr(centers), _lib.ptr(inbox), _lib.ptr(labels), _lib.ptr(targets), _lib.ptr(mask),
            _lib.stream_ptr()), 'sst_seg_targets_f32')
    return inbox, labels, targets, mask


def _box_centroids(points, inbox, boxes):
    """per-box mean of the member points (get_vote_target's scatter_v2(points, inbox_inds, 'avg')), without a host read: the
    library's deterministic segmented sum over ids 0..G (0 = background) with one sentinel row per id, so every box has a
    group.  The points are taken relative to their box's gravity centre, which keeps the fp32 sum of a box far from the origin
    as exact as one next to it."""
    from . import kernels as K
    n, g = points.size(0), boxes.size(0)
    dev = points.device
    gravity = torch.stack([boxes[:, 0], boxes[:, 1], boxes[:, 2] + boxes[:, 5] * 0.5], 1)
    member = (inbox >= 0).unsqueeze(1)
    rel = torch.where(member, points[:, :3] - gravity[inbox.clamp(min=0).long()], points.new_zeros(()))
    feats = torch.cat([rel, rel.new_zeros((g + 1, 3))]).contiguous()
    ids = torch.cat([inbox + 1, torch.arange(g + 1, dtype=torch.int32, device=dev)]).reshape(-1, 1).contiguous()
    plan = K.unique_rows(ids, [0], [g + 1], defer_count=True)
    plan.m = g + 1                                         # one sentinel per id: every id is a group
    sums = K.segment_reduce(feats, plan, 'sum')
    count = (plan.counts() - 1).clamp(min=1).to(torch.float32).unsqueeze(1)
    return (gravity + sums[1:] / count[1:]).contiguous()


@torch.no_grad()
def seg_point_targets(points_list, boxes_list, labels_list, bg_label, extra_width=None, centroid_offset=False):
    """-> (labels int64 [N], vote_targets fp32 [N, 3], vote_mask bool [N], inbox int32 [N]) of all samples concatenated.

    points_list: per sample [N_i, >= 3] fp32 device tensors (xyz first); boxes_list: [G_i, >= 7] tensors (x, y, z_bottom, w, l,
    h, rz) or objects with ``.tensor``; labels_list: [G_i] integer tensors, boxes with label < 0 are skipped.  ``inbox`` indexes
    the concatenated boxes.  Sample offsets come from the shapes: no synchronisation."""
    if not (len(points_list) == len(boxes_list) == len(labels_list)) or len(points_list) == 0:
        raise RuntimeError('seg_point_targets: one box set and one label set per sample expected')
    boxes_list = [b.tensor if hasattr(b, 'tensor') else b for b in boxes_list]
    dev = points_list[0].device
    for p, b, l in zip(points_list, boxes_list, labels_list):
        _check_f32(p)
        _lib.require_cuda(l)
        if b.numel():
            _check_f32(b.contiguous())
        if p.dim() != 2 or p.size(1) < 3 or b.dim() != 2 or (b.size(0) and b.size(1) < 7) or l.numel() != b.size(0):
            raise RuntimeError(f'seg_point_targets: points [N, >= 3], boxes [G, >= 7] and G labels expected, got '
                               f'{tuple(p.shape)}, {tuple(b.shape)}, {tuple(l.shape)}')
    points = points_list[0] if len(points_list) == 1 else torch.cat(points_list, 0)
    boxes = torch.cat([b[:, :7].to(dev) for b in boxes_list if b.size(0)], 0).contiguous() \
        if sum(b.size(0) for b in boxes_list) else points.new_zeros((0, 7))
    box_labels = torch.cat([l.reshape(-1).to(device=dev, dtype=torch.long) for l in labels_list]).contiguous()
    pt_off, _ = _offsets([p.size(0) for p in points_list], dev)
    box_off, _ = _offsets([b.size(0) for b in boxes_list], dev)
    batch = len(points_list)
    args = (points, pt_off, batch, boxes, box_labels, box_off, extra_width, bg_label)
    inbox, labels, targets, mask = _targets_launch(*args, None)
    if centroid_offset and boxes.size(0) > 0 and points.size(0) > 0:
        inbox, labels, targets, mask = _targets_launch(*args, _box_centroids(points, inbox, boxes))
    return labels, targets, mask.bool(), inbox


class _SegVoteLoss(torch.autograd.Function):

    @staticmethod
    def forward(ctx, logits, vote_preds, labels, vote_targets, vote_mask, cfg):
        n, c = logits.shape
        lib = _lib.load()
        dev = logits.device
        out = torch.empty(2 + c + 1, dtype=torch.float32, device=dev)
        counts = torch.empty(2 + 2 * c, dtype=torch.long, device=dev)
        ws = _lib.workspace(lib.sst_seg_loss_workspace_bytes(n, c), dev)
        _lib.check(lib.sst_seg_loss_fwd_f32(
            _lib.ptr(logits), _lib.ptr(vote_preds), _lib.ptr(labels), _lib.ptr(vote_targets), _lib.ptr(vote_mask), n, c,
            cfg['mode'], cfg['logit_scale'], cfg['gamma'], cfg['alpha'], _lib.ptr(cfg['class_weight']),
            _lib.ptr(cfg['score_thresh']), _lib.ptr(cfg['class_group']), cfg['n_groups'], _lib.ptr(out), _lib.ptr(counts),
            _lib.ptr(ws), _lib.stream_ptr()), 'sst_seg_loss_fwd_f32')
        ctx.save_for_backward(logits, vote_preds, labels, vote_targets, vote_mask, counts)
        ctx.cfg = cfg
        recall, num_fg = out[2:2 + c], out[2 + c:]
        ctx.mark_non_differentiable(recall, num_fg, counts)
        return out[0] * cfg['w_decode'], out[1] * cfg['w_vote'], recall, num_fg, counts

    @staticmethod
    def backward(ctx, g_sem, g_vote, *_unused):
        logits, vote_preds, labels, vote_targets, vote_mask, counts = ctx.saved_tensors
        cfg = ctx.cfg
        n, c = logits.shape
        zero = logits.new_zeros(())
        g = torch.stack([(zero if g_sem is None else g_sem.reshape(())) * cfg['w_decode'],
                         (zero if g_vote is None else g_vote.reshape(())) * cfg['w_vote']]).to(torch.float32).contiguous()
        d_logits = torch.empty_like(logits)
        d_votes = torch.empty_like(vote_preds)
        _lib.check(_lib.load().sst_seg_loss_bwd_f32(
            _lib.ptr(logits), _lib.ptr(vote_preds), _lib.ptr(labels), _lib.ptr(vote_targets), _lib.ptr(vote_mask), n, c,
            cfg['mode'], cfg['logit_scale'], cfg['gamma'], cfg['alpha'], _lib.ptr(cfg['class_weight']), _lib.ptr(g),
            _lib.ptr(counts), _lib.ptr(d_logits), _lib.ptr(d_votes), _lib.stream_ptr()), 'sst_seg_loss_bwd_f32')
        return d_logits, d_votes, None, None, None, None


def _device_vector(values, dtype, device, length, what):
    if values is None:
        return None
    t = values if torch.is_tensor(values) else torch.tensor(list(values), dtype=dtype)
    t = t.to(device=device, dtype=dtype, non_blocking=True).contiguous()
    if t.dim() != 1 or t.numel() != length:
        raise RuntimeError(f'seg_vote_loss: {what} needs {length} entries, got {tuple(t.shape)}')
    return t


def seg_vote_loss(logits, vote_preds, labels, vote_targets, vote_mask, *, mode, logit_scale=1.0, gamma=2.0, alpha=0.25,
                  class_weight=None, loss_weight_decode=1.0, loss_weight_vote=1.0, score_thresh=None, class_group=None):
    """-> (loss_sem * loss_weight_decode, loss_vote * loss_weight_vote, recall [C], num_fg [1], counts int64 [2 + 2C]).

    logits [N, C], vote_preds [N, 3C], labels int64 [N], vote_targets [N, 3], vote_mask bool / uint8 [N].  mode:
    SIGMOID_FOCAL (C classes, label C = background) or SOFTMAX_CE (the last class is the background; class_weight [C] optional).
    score_thresh: None (no statistics), C thresholds (sigmoid) or one per group with class_group [C - 1] (cross entropy).
    counts = (num_valid, status, tp per class, real per class); status: STATUS_BAD_LABEL | STATUS_MASKED_NO_CLASS.  The two
    losses carry gradients to logits and vote_preds (one launch); nothing is read back to the host."""
    if mode not in (SIGMOID_FOCAL, SOFTMAX_CE):
        raise RuntimeError(f'seg_vote_loss: unknown mode {mode}')
    _check_f32(logits, vote_preds, vote_targets)
    if logits.dim() != 2 or not 1 <= logits.size(1) <= 32 or logits.size(0) < 1:
        raise RuntimeError(f'seg_vote_loss: logits [N >= 1, 1 <= C <= 32] expected, got {tuple(logits.shape)}')
    n, c = logits.shape
    _check(vote_preds, torch.float32, (n, 3 * c), 'vote_preds')
    _check(vote_targets, torch.float32, (n, 3), 'vote_targets')
    _check(labels, torch.long, (n,), 'labels')
    if vote_mask.dtype == torch.bool:
        vote_mask = vote_mask.view(torch.uint8)
    _check(vote_mask, torch.uint8, (n,), 'vote_mask')
    dev = logits.device
    n_groups = 0
    thr = grp = None
    if score_thresh is not None:
        if mode == SIGMOID_FOCAL:
            thr = _device_vector(score_thresh, torch.float32, dev, c, 'score_thresh')
        else:
            n_groups = len(score_thresh)
            thr = _device_vector(score_thresh, torch.float32, dev, n_groups, 'score_thresh')
            grp = _device_vector(class_group, torch.int32, dev, c - 1, 'class_group')
            if grp is None:
                raise RuntimeError('seg_vote_loss: the cross-entropy statistics need class_group')
    cfg = dict(mode=int(mode), logit_scale=float(logit_scale), gamma=float(gamma), alpha=float(alpha),
               class_weight=_device_vector(class_weight, torch.float32, dev, c, 'class_weight') if mode == SOFTMAX_CE else None,
               score_thresh=thr, class_group=grp, n_groups=n_groups, w_decode=float(loss_weight_decode),
               w_vote=float(loss_weight_vote))
    return _SegVoteLoss.apply(logits, vote_preds, labels, vote_targets, vote_mask, cfg)
