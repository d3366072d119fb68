"""The second stage of FSD / FSDv2 (csrc/roi_head.hip): GroupCorrectionHead, FullySparseBboxHead and DeltaXYZWLHRBBoxCoder.

Reference: mmdet3d/models/roi_heads/fsd_roi_head.py, roi_heads/bbox_heads/fsd_bbox_head.py, core/bbox/samplers/
iou_neg_piecewise_sampler.py, core/bbox/coders/delta_xyzwhlr_bbox_coder.py and mmdet's MaxIoUAssigner.  The network (six
``SIRLayer`` blocks and the two MLP heads) is built from the library's modules; what the reference runs around it on the host is
five kernels' work here: ``roi_assign_sample`` (two launches for all samples and classes instead of, per sample and class, two
mask compactions, an IoU launch, the assigner's Python loop over boxes, and ``nonzero`` / ``randperm`` / ``unique`` in the
sampler, then per sample the canonical transform and the encode), ``roi_loss`` (two launches forward, one backward: no
``.item()``, no per-sample re-compaction, no thirty-op corner loss for autograd to replay) and ``roi_decode`` (one launch).
fp32 device tensors only; CPU, non-fp32 or non-contiguous inputs raise.
"""
import ctypes
import functools

import torch
from torch import nn
from torch.nn import functional as F

from . import _head_common
from . import _lib
from . import box_ops
from ._head_common import LOSS_COUNTS, LOSS_FINISH, cfg_get as _cfg_get, offsets as _offsets
from .center_head import BBOX_CODERS, build_bbox_coder
from .detectors import HEADS, build_head
from .registry import ROI_EXTRACTORS, build_voxel_encoder
from .sst_ops import build_mlp

MAX_CLASSES, MAX_PIECES = 16, 8

_check_f32 = functools.partial(_head_common.check_f32, 'sst_amd.roi_head')
_check = functools.partial(_head_common.check, 'sst_amd.roi_head')


def roi_assign_gt_tile():
    """ground-truth boxes per LDS tile of the assignment kernel (a sample with more boxes crosses tiles)"""
    return int(_lib.load().sst_roi_assign_gt_tile())


def roi_assign_block():
    """proposals per workgroup of the assignment kernel"""
    return int(_lib.load().sst_roi_assign_block())


def roi_sample_max_proposals():
    """proposals of one sample the sampling kernel holds in LDS"""
    return int(_lib.load().sst_roi_sample_max_proposals())


def _per_class(value, n, what):
    vals = [float(v) for v in value] if isinstance(value, (list, tuple)) else [float(value)] * n
    if len(vals) != n:
        raise RuntimeError(f'roi_assign_sample: {what} needs {n} entries, got {len(vals)}')
    return vals


def _fill(arr, vals):
    for i, v in enumerate(vals):
        arr[i] = v


@torch.no_grad()
def roi_assign_sample(proposals, proposal_labels, gt_bboxes, gt_labels, *, num_classes, pos_iou_thr, neg_iou_thr, min_pos_iou,
                      num, pos_fraction, neg_piece_fractions, neg_iou_piece_thrs, cls_pos_thr, cls_neg_thr, class_mask=True,
                      keys=None, generator=None):
    """_assign_and_sample + get_targets of the reference for all samples: two launches, nothing read back.

    proposals / proposal_labels / gt_bboxes / gt_labels: per sample an fp32 [P_i, 7 | 9] tensor (or an object with ``.tensor``),
    int64 [P_i], fp32 [G_i, >= 7], int64 [G_i].  A sample without a proposal gets the reference's fake box (0, 0, 5, 1, 1, 1, 0
    [, 0, 0]) with label 0.  pos_iou_thr / neg_iou_thr / min_pos_iou: per class (the list of per-class assigners, class_mask
    True) or one float (the single assigner, class_mask False).  keys: fp32 [sum P_i] (fake boxes included), one per proposal;
    default ``torch.rand`` under ``generator``.  "k of a pool" = its k smallest (key, index).

    -> dict of device tensors.  Per sample ``num`` rows, positives first, each group in ascending proposal index, padded:
    rois [B num, 1 + cols], src int32 (index into the concatenated proposals), gt_index int32 (into the concatenated boxes),
    labels int64, iou, soft_label, reg_mask uint8, targets [B num, 7], counts int32 [B, 2] = (positives, negatives); and the
    intermediate overlaps [P, ld] (-1 where masked), max_overlaps [P], argmax int32 [P], assigned int32 [P] (-1 background, -2
    ignored), keys, proposals / proposal_labels / gts / gt_labels (concatenated) and the host lists prop_lens / gt_lens."""
    batch = len(proposals)
    if batch == 0 or not (batch == len(proposal_labels) == len(gt_bboxes) == len(gt_labels)):
        raise RuntimeError('roi_assign_sample: per sample one tensor of each kind expected')
    props = [p.tensor if hasattr(p, 'tensor') else p for p in proposals]
    gts = [g.tensor if hasattr(g, 'tensor') else g for g in gt_bboxes]
    _check_f32(*props)
    dev = props[0].device
    cols = {p.size(1) for p in props}
    if len(cols) != 1 or not cols <= {7, 9} or any(p.dim() != 2 for p in props):
        raise RuntimeError(f'roi_assign_sample: proposals of 7 or 9 columns expected, got {[tuple(p.shape) for p in props]}')
    cols = cols.pop()
    plabels = list(proposal_labels)
    for s in range(batch):
        if props[s].size(0) == 0:       # fsd_roi_head.py:232-241
            fake = [0, 0, 5, 1, 1, 1, 0] + [0] * (cols - 7)
            props[s] = torch.tensor([fake], dtype=torch.float32).to(dev, non_blocking=True)
            plabels[s] = torch.zeros(1, dtype=torch.long).to(dev, non_blocking=True)
        if plabels[s].numel() != props[s].size(0):
            raise RuntimeError('roi_assign_sample: one label per proposal expected')
    gcols = {g.size(1) for g in gts if g.size(0)}
    if len(gcols) > 1 or any(c < 7 for c in gcols):
        raise RuntimeError(f'roi_assign_sample: boxes of one width >= 7 expected, got {sorted(gcols)}')
    gcols = gcols.pop() if gcols else 7
    filled = [g.to(dev) for g in gts if g.size(0)]
    _check_f32(*filled)
    gt = torch.cat(filled, 0).contiguous() if filled else torch.zeros((0, gcols), dtype=torch.float32, device=dev)
    glab = torch.cat([l.reshape(-1).to(device=dev, dtype=torch.long) for l in gt_labels]).contiguous()
    if glab.numel() != gt.size(0):
        raise RuntimeError('roi_assign_sample: one label per box expected')
    prop = torch.cat(props, 0).contiguous()
    plab = torch.cat([l.reshape(-1).to(device=dev, dtype=torch.long) for l in plabels]).contiguous()
    prop_lens, gt_lens = [p.size(0) for p in props], [g.size(0) for g in gts]
    prop_off, gt_off = _offsets(prop_lens, dev)[0], _offsets(gt_lens, dev)[0]
    n_props, n_gts, ld = prop.size(0), gt.size(0), max(gt_lens)
    if not 1 <= num_classes <= MAX_CLASSES:
        raise RuntimeError(f'roi_assign_sample: 1 to {MAX_CLASSES} classes, got {num_classes}')
    n_thr = num_classes if class_mask else 1
    pos_thr, neg_thr = _per_class(pos_iou_thr, n_thr, 'pos_iou_thr'), _per_class(neg_iou_thr, n_thr, 'neg_iou_thr')
    min_pos = _per_class(min_pos_iou, n_thr, 'min_pos_iou')
    cpos, cneg = _per_class(cls_pos_thr, num_classes, 'cls_pos_thr'), _per_class(cls_neg_thr, num_classes, 'cls_neg_thr')
    fracs, pieces = [float(v) for v in neg_piece_fractions], [float(v) for v in neg_iou_piece_thrs]
    if len(fracs) != len(pieces) or not 1 <= len(pieces) <= MAX_PIECES:
        raise RuntimeError(f'roi_assign_sample: 1 to {MAX_PIECES} negative pieces with one fraction each expected')
    if keys is None:
        keys = torch.rand(n_props, dtype=torch.float32, device=dev, generator=generator)
    _check(keys, torch.float32, (n_props,), 'keys')

    lib = _lib.load()
    iou = torch.empty((n_props, ld), dtype=torch.float32, device=dev)
    max_iou = torch.empty(n_props, dtype=torch.float32, device=dev)
    argmax = torch.empty(n_props, dtype=torch.int32, device=dev)
    a = _lib.RoiAssignArgs()
    a.props, a.prop_labels, a.prop_offsets = prop.data_ptr(), plab.data_ptr(), prop_off.data_ptr()
    a.gts, a.gt_labels, a.gt_offsets = gt.data_ptr(), glab.data_ptr(), gt_off.data_ptr()
    a.iou, a.max_iou, a.argmax = iou.data_ptr(), max_iou.data_ptr(), argmax.data_ptr()
    a.n_props, a.n_gts, a.ld = n_props, n_gts, ld
    a.prop_cols, a.gt_cols, a.batch, a.num_classes, a.class_mask = cols, gcols, batch, int(num_classes), 1 if class_mask else 0
    _lib.check(lib.sst_roi_assign_f32(ctypes.byref(a), _lib.stream_ptr()), 'sst_roi_assign_f32')

    rows = batch * int(num)
    out = dict(rois=torch.empty((rows, 1 + cols), dtype=torch.float32, device=dev),
               src=torch.empty(rows, dtype=torch.int32, device=dev), gt_index=torch.empty(rows, dtype=torch.int32, device=dev),
               labels=torch.empty(rows, dtype=torch.long, device=dev), iou=torch.empty(rows, dtype=torch.float32, device=dev),
               soft_label=torch.empty(rows, dtype=torch.float32, device=dev),
               reg_mask=torch.empty(rows, dtype=torch.uint8, device=dev),
               targets=torch.empty((rows, 7), dtype=torch.float32, device=dev),
               counts=torch.empty((batch, 2), dtype=torch.int32, device=dev))
    assigned = torch.empty(n_props, dtype=torch.int32, device=dev)
    b = _lib.RoiSampleArgs()
    b.props, b.prop_labels, b.prop_offsets = prop.data_ptr(), plab.data_ptr(), prop_off.data_ptr()
    b.gts, b.gt_labels, b.gt_offsets = gt.data_ptr(), glab.data_ptr(), gt_off.data_ptr()
    b.iou, b.max_iou, b.argmax, b.keys, b.assigned = (iou.data_ptr(), max_iou.data_ptr(), argmax.data_ptr(), keys.data_ptr(),
                                                     assigned.data_ptr())
    b.rois, b.src, b.gt_index, b.labels = (out['rois'].data_ptr(), out['src'].data_ptr(), out['gt_index'].data_ptr(),
                                           out['labels'].data_ptr())
    b.iou_out, b.soft_label, b.reg_mask = out['iou'].data_ptr(), out['soft_label'].data_ptr(), out['reg_mask'].data_ptr()
    b.targets, b.counts = out['targets'].data_ptr(), out['counts'].data_ptr()
    b.n_props, b.n_gts, b.ld, b.max_props_per_sample = n_props, n_gts, ld, max(prop_lens)
    b.prop_cols, b.gt_cols, b.batch, b.num_classes, b.class_mask = cols, gcols, batch, int(num_classes), 1 if class_mask else 0
    b.num, b.num_expected_pos, b.n_pieces = int(num), int(num * pos_fraction), len(pieces)
    _fill(b.pos_iou_thr, pos_thr)
    _fill(b.neg_iou_thr, neg_thr)
    _fill(b.min_pos_iou, min_pos)
    _fill(b.piece_thr, pieces)
    _fill(b.cls_pos_thr, cpos)
    _fill(b.cls_neg_thr, cneg)
    _fill(b.piece_frac, fracs)
    _lib.check(lib.sst_roi_sample_targets_f32(ctypes.byref(b), _lib.stream_ptr()), 'sst_roi_sample_targets_f32')
    out.update(overlaps=iou, max_overlaps=max_iou, argmax=argmax, assigned=assigned, keys=keys, proposals=prop,
               proposal_labels=plab, gts=gt, gt_labels=glab, prop_lens=prop_lens, gt_lens=gt_lens, num=int(num))
    return out


ROW_KEYS = ('rois', 'src', 'gt_index', 'labels', 'iou', 'soft_label', 'reg_mask', 'targets')


def roi_compact(samples):
    """drop the padding rows of ``roi_assign_sample``: reads ``counts`` once (B x 2 integers, the one host read of the training
    step outside the extractor's own) -> the same dict with the concatenated rows of all samples and ``counts`` as a host list"""
    counts = samples['counts'].tolist()
    num = samples['num']
    for s, (n_pos, n_neg) in enumerate(counts):
        if n_pos < 0:
            raise RuntimeError(f'roi_assign_sample: sample {s} has more than {roi_sample_max_proposals()} proposals')
    dev = samples['rois'].device
    rows = torch.cat([torch.arange(s * num, s * num + n_pos + n_neg) for s, (n_pos, n_neg) in enumerate(counts)])
    rows = rows.to(dev, non_blocking=True)
    out = dict(samples)
    for k in ROW_KEYS:
        out[k] = samples[k][rows]
    out['counts'] = counts
    return out


class _RoiLoss(torch.autograd.Function):

    @staticmethod
    def forward(ctx, cfg, cls_score, bbox_pred, nonempty, rois, soft_label, reg_mask, targets, gt_index, labels, gts):
        n = bbox_pred.size(0)
        dev = bbox_pred.device
        lib = _lib.load()
        out = torch.empty(5, dtype=torch.float32, device=dev)
        counts = torch.empty(4, dtype=torch.float64, device=dev)
        ws = _lib.workspace(lib.sst_roi_loss_workspace_bytes(n), dev)
        args = _loss_args(cfg, cls_score, bbox_pred, nonempty, rois, soft_label, reg_mask, targets, gt_index, labels, gts)

        def launch(phases):
            _lib.check(lib.sst_roi_loss_fwd_f32(ctypes.byref(args), phases, _lib.ptr(out), _lib.ptr(counts), _lib.ptr(ws),
                                                _lib.stream_ptr()), 'sst_roi_loss_fwd_f32')

        dist = torch.distributed
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        sync = [k for k, on in ((2, cfg['sync_cls']), (3, cfg['sync_reg'])) if on]
        if world > 1 and sync:
            # reduce_mean of the averaging factors, on the device: counts is written by the first call and read by the second
            launch(LOSS_COUNTS)
            avg = counts[sync].contiguous()
            dist.all_reduce(avg.div_(world))
            counts[sync] = avg
            launch(LOSS_FINISH)
        else:
            launch(LOSS_COUNTS | LOSS_FINISH)
        ctx.save_for_backward(counts, cls_score, bbox_pred, nonempty, rois, soft_label, reg_mask, targets, gt_index, labels, gts)
        ctx.cfg = cfg
        ctx.mark_non_differentiable(counts)
        ctx.set_materialize_grads(False)
        num = out[3:5].clone()
        ctx.mark_non_differentiable(num)
        return out[0], out[1], out[2], num, counts

    @staticmethod
    def backward(ctx, g_cls, g_bbox, g_corner, _g_num, _g_counts):
        counts, cls_score, bbox_pred, *rest = ctx.saved_tensors
        zero = bbox_pred.new_zeros(())
        g = torch.stack([zero if x is None else x.reshape(()).to(torch.float32) for x in (g_cls, g_bbox, g_corner)])
        d_cls, d_bbox = torch.empty_like(cls_score), torch.empty_like(bbox_pred)
        args = _loss_args(ctx.cfg, cls_score, bbox_pred, *rest)
        _lib.check(_lib.load().sst_roi_loss_bwd_f32(ctypes.byref(args), _lib.ptr(g), _lib.ptr(counts), _lib.ptr(d_cls),
                                                    _lib.ptr(d_bbox), _lib.stream_ptr()), 'sst_roi_loss_bwd_f32')
        return (None, d_cls, d_bbox) + (None,) * 8


def _loss_args(cfg, cls_score, bbox_pred, nonempty, rois, soft_label, reg_mask, targets, gt_index, labels, gts):
    a = _lib.RoiLossArgs()
    a.cls_score, a.bbox_pred, a.nonempty, a.rois = cls_score.data_ptr(), bbox_pred.data_ptr(), nonempty.data_ptr(), rois.data_ptr()
    a.soft_label, a.reg_mask, a.targets = soft_label.data_ptr(), reg_mask.data_ptr(), targets.data_ptr()
    a.gt_index, a.labels, a.gts = gt_index.data_ptr(), labels.data_ptr(), gts.data_ptr() if gts.numel() else None
    a.n, a.n_gts, a.roi_cols, a.gt_cols = bbox_pred.size(0), gts.size(0), rois.size(1), gts.size(1)
    a.with_corner, a.car_index, a.beta = 1 if cfg['with_corner'] else 0, cfg['car_index'], cfg['beta']
    a.w_cls, a.w_reg, a.w_corner = cfg['loss_weights']
    _fill(a.code_weight, cfg['code_weight'])
    return a


def roi_loss(cls_score, bbox_pred, nonempty_roi_mask, rois, soft_label, reg_mask, targets, gt_index=None, labels=None, gts=None, *,
             loss_weights=(1.0, 1.0, 1.0), smooth_l1_beta=0.0, code_weight=None, with_corner_loss=False, car_index=-1,
             sync_cls_avg_factor=False, sync_reg_avg_factor=False):
    """FullySparseBboxHead.loss -> (loss_rcnn_cls, loss_rcnn_bbox, loss_rcnn_corner, (num_pos_rois, num_neg_rois) fp32 [2],
    counts float64 [4] = (num_pos, corner rows, cls_avg, reg_avg)): two launches forward, one backward, nothing read back.

    cls_score [R, 1], bbox_pred [R, 7], nonempty_roi_mask bool | uint8 [R], rois [R, 8 | 10] = (sample, box), soft_label [R],
    reg_mask uint8 [R], targets [R, 7] as ``roi_compact(roi_assign_sample(...))`` gives them; for the corner loss gt_index int32
    [R], labels int64 [R] and the concatenated boxes gts [G, >= 7].  loss_weights: (cls, bbox, corner);  smooth_l1_beta > 0: mmdet's
    SmoothL1Loss, 0: L1Loss;  car_index >= 0: the corner loss only on rows of that class (corner_loss_only_car)."""
    _check_f32(cls_score, bbox_pred, rois, soft_label, targets)
    n = bbox_pred.size(0)
    if bbox_pred.dim() != 2 or bbox_pred.size(1) != 7 or n == 0:
        raise RuntimeError(f'roi_loss: bbox_pred [R >= 1, 7] expected, got {tuple(bbox_pred.shape)}')
    if cls_score.numel() != n or rois.dim() != 2 or rois.size(0) != n or rois.size(1) not in (8, 10):
        raise RuntimeError(f'roi_loss: cls_score [R, 1] and rois [R, 8 | 10] expected, got {tuple(cls_score.shape)}, {tuple(rois.shape)}')
    _check(soft_label, torch.float32, (n,), 'soft_label')
    _check(targets, torch.float32, (n, 7), 'targets')
    _check(reg_mask, torch.uint8, (n,), 'reg_mask')
    _lib.require_cuda(nonempty_roi_mask)
    nonempty = nonempty_roi_mask.view(torch.uint8) if nonempty_roi_mask.dtype == torch.bool else nonempty_roi_mask
    _check(nonempty, torch.uint8, (n,), 'nonempty_roi_mask')
    dev = bbox_pred.device
    if with_corner_loss:
        if gt_index is None or labels is None or gts is None:
            raise RuntimeError('roi_loss: the corner loss needs gt_index, labels and gts')
        _check(gt_index, torch.int32, (n,), 'gt_index')
        _check(labels, torch.long, (n,), 'labels')
        _check_f32(gts)
        if gts.dim() != 2 or gts.size(1) < 7:
            raise RuntimeError(f'roi_loss: gts [G, >= 7] expected, got {tuple(gts.shape)}')
    else:
        gt_index = torch.empty(0, dtype=torch.int32, device=dev) if gt_index is None else gt_index
        labels = torch.empty(0, dtype=torch.long, device=dev) if labels is None else labels
        gts = torch.empty((0, 7), dtype=torch.float32, device=dev) if gts is None else gts
    if code_weight is not None and len(code_weight) != 7:
        raise RuntimeError(f'roi_loss: code_weight needs 7 entries, got {len(code_weight)}')
    cfg = dict(loss_weights=[float(v) for v in loss_weights], beta=float(smooth_l1_beta),
               code_weight=[1.0] * 7 if code_weight is None else [float(v) for v in code_weight],
               with_corner=bool(with_corner_loss), car_index=int(car_index), sync_cls=bool(sync_cls_avg_factor),
               sync_reg=bool(sync_reg_avg_factor))
    return _RoiLoss.apply(cfg, cls_score, bbox_pred, nonempty, rois, soft_label, reg_mask, targets, gt_index, labels, gts)


@torch.no_grad()
def roi_decode(rois, bbox_pred, cls_score=None, with_bev=True):
    """-> (boxes [R, 7 | 9], scores [R] or None, bev [R, 5] or None) in one launch: decode_from_rois (fsd_bbox_head.py:634-653;
    the velocity of a 9-column RoI passes through), sigmoid(cls_score) and the rows xywhr2xyxyr(boxes.bev) gives for the NMS."""
    _check_f32(rois, bbox_pred, cls_score)
    n = rois.size(0)
    if rois.dim() != 2 or rois.size(1) not in (8, 10) or tuple(bbox_pred.shape) != (n, 7):
        raise RuntimeError(f'roi_decode: rois [R, 8 | 10] and bbox_pred [R, 7] expected, got {tuple(rois.shape)}, '
                           f'{tuple(bbox_pred.shape)}')
    if cls_score is not None and cls_score.numel() != n:
        raise RuntimeError(f'roi_decode: cls_score [R, 1] expected, got {tuple(cls_score.shape)}')
    dev = rois.device
    boxes = torch.empty((n, rois.size(1) - 1), dtype=torch.float32, device=dev)
    scores = torch.empty(n, dtype=torch.float32, device=dev) if cls_score is not None else None
    bev = torch.empty((n, 5), dtype=torch.float32, device=dev) if with_bev else None
    _lib.check(_lib.load().sst_roi_decode_f32(_lib.ptr(rois), rois.size(1), _lib.ptr(bbox_pred), _lib.ptr(cls_score), n,
                                              _lib.ptr(boxes), _lib.ptr(scores), _lib.ptr(bev), _lib.stream_ptr()),
               'sst_roi_decode_f32')
    return boxes, scores, bev


@BBOX_CODERS.register_module()
class DeltaXYZWLHRBBoxCoder(object):
    """core/bbox/coders/delta_xyzwhlr_bbox_coder.py: the reference's torch arithmetic (any device, differentiable).  The head's
    hot paths do not come through here: the encode of the targets is part of ``roi_assign_sample``, the decodes are part of
    ``roi_loss`` and ``roi_decode``."""

    def __init__(self, code_size=7):
        self.code_size = code_size

    @staticmethod
    def encode(src_boxes, dst_boxes):
        xa, ya, za, wa, la, ha, ra, *cas = torch.split(src_boxes, 1, dim=-1)
        xg, yg, zg, wg, lg, hg, rg, *cgs = torch.split(dst_boxes, 1, dim=-1)
        cts = [g - a for g, a in zip(cgs, cas)]
        za = za + ha / 2
        zg = zg + hg / 2
        diagonal = torch.sqrt(la**2 + wa**2)
        xt = (xg - xa) / diagonal
        yt = (yg - ya) / diagonal
        zt = (zg - za) / ha
        lt = torch.log(lg / la)
        wt = torch.log(wg / wa)
        ht = torch.log(hg / ha)
        rt = rg - ra
        return torch.cat([xt, yt, zt, wt, lt, ht, rt, *cts], dim=-1)

    @staticmethod
    def decode(anchors, deltas):
        xa, ya, za, wa, la, ha, ra, *cas = torch.split(anchors, 1, dim=-1)
        xt, yt, zt, wt, lt, ht, rt, *cts = torch.split(deltas, 1, dim=-1)
        za = za + ha / 2
        diagonal = torch.sqrt(la**2 + wa**2)
        xg = xt * diagonal + xa
        yg = yt * diagonal + ya
        zg = zt * ha + za
        lg = torch.exp(lt) * la
        wg = torch.exp(wt) * wa
        hg = torch.exp(ht) * ha
        rg = rt + ra
        zg = zg - hg / 2
        cgs = [t + a for t, a in zip(cts, cas)]
        return torch.cat([xg, yg, zg, wg, lg, hg, rg, *cgs], dim=-1)


def _parse_assigner(assigner, num_classes):
    """-> (class_mask, pos_iou_thr, neg_iou_thr, min_pos_iou); refuses what the kernels do not do, by name"""
    per_class = isinstance(assigner, (list, tuple))
    cfgs = list(assigner) if per_class else [assigner]
    if per_class and len(cfgs) != num_classes:
        raise NotImplementedError(f'GroupCorrectionHead: assigner: {len(cfgs)} assigners for {num_classes} classes')
    for cfg in cfgs:
        if _cfg_get(cfg, 'type') != 'MaxIoUAssigner':
            raise NotImplementedError(f'GroupCorrectionHead: assigner type {_cfg_get(cfg, "type")!r}: only MaxIoUAssigner is built')
        calc = _cfg_get(cfg, 'iou_calculator', dict(type='BboxOverlaps2D'))
        if _cfg_get(calc, 'type') != 'BboxOverlaps3D' or _cfg_get(calc, 'coordinate') != 'lidar':
            raise NotImplementedError(f'GroupCorrectionHead: iou_calculator {dict(calc)}: only BboxOverlaps3D with coordinate '
                                      f'\'lidar\' is built')
        if _cfg_get(cfg, 'ignore_iof_thr', -1) > 0:
            raise NotImplementedError('GroupCorrectionHead: ignore_iof_thr > 0 is not built')
        for key, default in (('gt_max_assign_all', True), ('match_low_quality', True)):
            if _cfg_get(cfg, key, default) is not default:
                raise NotImplementedError(f'GroupCorrectionHead: {key}={_cfg_get(cfg, key)} is not built')
        if isinstance(_cfg_get(cfg, 'neg_iou_thr'), (list, tuple)):
            raise NotImplementedError('GroupCorrectionHead: the tuple form of neg_iou_thr is not built')
    return (per_class, [float(c['pos_iou_thr']) for c in cfgs], [float(c['neg_iou_thr']) for c in cfgs],
            [float(_cfg_get(c, 'min_pos_iou', 0.0)) for c in cfgs])


def _parse_sampler(cfg):
    if _cfg_get(cfg, 'type') != 'IoUNegPiecewiseSampler':
        raise NotImplementedError(f'GroupCorrectionHead: sampler type {_cfg_get(cfg, "type")!r}: only IoUNegPiecewiseSampler is built')
    if _cfg_get(cfg, 'add_gt_as_proposals', False):
        raise NotImplementedError('GroupCorrectionHead: add_gt_as_proposals=True is not built')
    if _cfg_get(cfg, 'neg_pos_ub', -1) >= 0:
        raise NotImplementedError('GroupCorrectionHead: neg_pos_ub >= 0 is not built')
    if not _cfg_get(cfg, 'return_iou', False):
        raise NotImplementedError('GroupCorrectionHead: return_iou=False: the head\'s soft labels need the IoU')
    return dict(num=int(cfg['num']), pos_fraction=float(cfg['pos_fraction']),
                neg_piece_fractions=list(cfg['neg_piece_fractions']), neg_iou_piece_thrs=list(cfg['neg_iou_piece_thrs']))


@HEADS.register_module()
class FullySparseBboxHead(nn.Module):
    """roi_heads/bbox_heads/fsd_bbox_head.py:20-790 with the reference's constructor signature, module tree and order of RNG
    draws.  ``forward`` is the reference's; ``get_targets`` hands on what ``roi_assign_sample`` made, ``loss`` is the fused
    ``roi_loss``, ``get_bboxes`` decodes with ``roi_decode`` and runs the library's NMS."""

    def __init__(self, num_classes, num_blocks, in_channels, feat_channels, rel_mlp_hidden_dims, rel_mlp_in_channels, reg_mlp,
                 cls_mlp, with_rel_mlp=True, with_cluster_center=False, with_distance=False, mode='max',
                 xyz_normalizer=[20, 20, 4], act='gelu', geo_input=True, with_corner_loss=False,
                 bbox_coder=dict(type='DeltaXYZWLHRBBoxCoder'), norm_cfg=dict(type='LN', eps=1e-3, momentum=0.01),
                 corner_loss_weight=1.0, loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=2.0),
                 loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, reduction='none', loss_weight=1.0), dropout=0,
                 cls_dropout=0, reg_dropout=0, unique_once=False, init_cfg=None, train_cfg=None, test_cfg=None):
        super().__init__()
        if _cfg_get(bbox_coder, 'type') != 'DeltaXYZWLHRBBoxCoder' or _cfg_get(bbox_coder, 'code_size', 7) != 7:
            raise NotImplementedError(f'FullySparseBboxHead: bbox_coder {dict(bbox_coder)}: only DeltaXYZWLHRBBoxCoder with '
                                      f'code_size 7 is built')
        if _cfg_get(loss_cls, 'type') != 'CrossEntropyLoss' or not _cfg_get(loss_cls, 'use_sigmoid', False) \
                or _cfg_get(loss_cls, 'reduction', 'mean') != 'mean' or _cfg_get(loss_cls, 'class_weight') is not None:
            raise NotImplementedError(f'FullySparseBboxHead: loss_cls {dict(loss_cls)}: only the sigmoid CrossEntropyLoss with mean '
                                      f'reduction is built')
        if _cfg_get(loss_bbox, 'type') not in ('L1Loss', 'SmoothL1Loss') or _cfg_get(loss_bbox, 'reduction', 'mean') != 'mean':
            raise NotImplementedError(f'FullySparseBboxHead: loss_bbox {dict(loss_bbox)}: only L1Loss and SmoothL1Loss with mean '
                                      f'reduction are built')
        self.smooth_l1_beta = float(_cfg_get(loss_bbox, 'beta', 1.0)) if loss_bbox['type'] == 'SmoothL1Loss' else 0.0
        if loss_bbox['type'] == 'SmoothL1Loss' and not self.smooth_l1_beta > 0:
            raise NotImplementedError(f'FullySparseBboxHead: loss_bbox {dict(loss_bbox)}: SmoothL1Loss needs beta > 0')
        self.num_classes = num_classes
        self.with_corner_loss = with_corner_loss
        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.box_code_size = self.bbox_coder.code_size
        self.loss_weights = [float(_cfg_get(loss_cls, 'loss_weight', 1.0)), float(_cfg_get(loss_bbox, 'loss_weight', 1.0)),
                             float(corner_loss_weight)]
        self.use_sigmoid_cls = True
        self.geo_input = geo_input
        self.corner_loss_weight = corner_loss_weight
        self.num_blocks = num_blocks
        self.print_info = {}
        self.unique_once = unique_once
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.fp16_enabled = False

        block_list = []
        for i in range(num_blocks):
            block_list.append(build_voxel_encoder(dict(
                type='SIRLayer', in_channels=in_channels[i], feat_channels=feat_channels[i], with_distance=with_distance,
                with_cluster_center=with_cluster_center, with_rel_mlp=with_rel_mlp, rel_mlp_hidden_dims=rel_mlp_hidden_dims[i],
                rel_mlp_in_channel=rel_mlp_in_channels[i], with_voxel_center=False, voxel_size=[0.1, 0.1, 0.1],
                point_cloud_range=[-74.88, -74.88, -2, 74.88, 74.88, 4], norm_cfg=norm_cfg, mode=mode, fusion_layer=None,
                return_point_feats=i != num_blocks - 1, return_inv=False, rel_dist_scaler=10.0, xyz_normalizer=xyz_normalizer,
                act=act, dropout=dropout)))
        self.block_list = nn.ModuleList(block_list)
        end_channel = sum(sum(c) for c in feat_channels)
        if cls_mlp is not None:
            self.conv_cls = build_mlp(end_channel, list(cls_mlp) + [1, ], norm_cfg, True, act=act, dropout=cls_dropout)
        else:
            self.conv_cls = nn.Linear(end_channel, 1)
        if reg_mlp is not None:
            self.conv_reg = build_mlp(end_channel, list(reg_mlp) + [self.box_code_size, ], norm_cfg, True, act=act,
                                      dropout=reg_dropout)
        else:
            self.conv_reg = nn.Linear(end_channel, self.box_code_size)

    def forward(self, pts_xyz, pts_features, pts_info, roi_inds, rois):
        """-> (cls_score [R, 1], bbox_pred [R, 7], nonempty_roi_mask bool [R]) (fsd_bbox_head.py:117-173)"""
        assert pts_features.size(0) > 0
        pts_features, rois = _lib.as_fp32(pts_features, rois)       # force_fp32
        rois = rois[:, 1:]
        rel_xyz = pts_xyz[:, :3] - rois[:, :3][roi_inds]
        if self.unique_once:
            new_coors, unq_inv = torch.unique(roi_inds, return_inverse=True, return_counts=False, dim=0)
        else:
            new_coors = unq_inv = None
        out_feats = pts_features
        f_cluster = torch.cat([pts_info['local_xyz'], pts_info['boundary_offset'], pts_info['is_in_margin'][:, None], rel_xyz], dim=-1)
        cluster_feat_list = []
        for i, block in enumerate(self.block_list):
            in_feats = torch.cat([pts_xyz, out_feats], 1)
            if self.geo_input:
                in_feats = torch.cat([in_feats, f_cluster / 10], 1)
            if i < self.num_blocks - 1:
                out_feats, out_cluster_feats = block(in_feats, roi_inds, f_cluster, unq_inv_once=unq_inv, new_coors_once=new_coors)
            else:
                out_cluster_feats, out_coors = block(in_feats, roi_inds, f_cluster, unq_inv_once=unq_inv, new_coors_once=new_coors)
            cluster_feat_list.append(out_cluster_feats)
        final_cluster_feats = torch.cat(cluster_feat_list, dim=1)
        # the groups come sorted (torch.unique), the empty group -1 first: the reference's training-time asserts (:162-163,
        # :176-180) restate this and cost four read-backs; they are not repeated here
        nonempty_roi_mask = self.get_nonempty_roi_mask(out_coors, len(rois))
        cls_score = self.conv_cls(final_cluster_feats)
        bbox_pred = self.conv_reg(final_cluster_feats)
        cls_score = self.align_roi_feature_and_rois(cls_score, out_coors, len(rois))
        bbox_pred = self.align_roi_feature_and_rois(bbox_pred, out_coors, len(rois))
        return cls_score, bbox_pred, nonempty_roi_mask

    def get_nonempty_roi_mask(self, out_coors, num_rois):
        """no compaction: the group -1 (points of no RoI) writes a spare last element"""
        mask = torch.zeros(num_rois + 1, dtype=torch.bool, device=out_coors.device)
        mask[torch.where(out_coors >= 0, out_coors, out_coors.new_full((), num_rois))] = True
        return mask[:num_rois]

    def align_roi_feature_and_rois(self, features, out_coors, num_rois):
        """scatter the group rows to their RoIs (:186-204) without the mask compaction and its read-backs: the rows of the
        group -1 go to a spare last row.  Without any non-empty group every row is 0 either way (the reference's pseudo
        gradient), and the parameters still reach the graph."""
        new_feature = features.new_zeros((num_rois + 1, features.size(1)))
        index = torch.where(out_coors >= 0, out_coors, out_coors.new_full((), num_rois))
        new_feature = new_feature.index_copy(0, index, features)
        return new_feature[:num_rois]

    def get_targets(self, sampling_results, rcnn_train_cfg=None, concat=True):
        """``sampling_results``: what ``GroupCorrectionHead._assign_and_sample`` returned - the targets are already in it (the
        sampling kernel writes them); the padding is dropped here with the one read of ``counts``"""
        assert concat
        return sampling_results if isinstance(sampling_results['counts'], list) else roi_compact(sampling_results)

    def _car_index(self):
        if not _cfg_get(self.train_cfg, 'corner_loss_only_car', True):
            return -1
        return list(self.train_cfg['class_names']).index('Car')

    def loss(self, cls_score, bbox_pred, nonempty_roi_mask, rois, targets):
        """-> dict(loss_rcnn_cls, loss_rcnn_bbox, num_pos_rois, num_neg_rois [, loss_rcnn_corner]) (:207-330); ``targets``: the
        dict ``get_targets`` returned"""
        assert cls_score.shape[0] > 0
        cls_score, bbox_pred = _lib.as_fp32(cls_score).contiguous(), _lib.as_fp32(bbox_pred).contiguous()
        code_weights = _cfg_get(self.train_cfg, 'rcnn_code_weights', None)
        loss_cls, loss_bbox, loss_corner, num, counts = roi_loss(
            cls_score, bbox_pred, nonempty_roi_mask, rois.contiguous(), targets['soft_label'], targets['reg_mask'],
            targets['targets'], targets['gt_index'], targets['labels'], targets['gts'], loss_weights=self.loss_weights,
            smooth_l1_beta=self.smooth_l1_beta, code_weight=list(code_weights) if code_weights is not None else None,
            with_corner_loss=self.with_corner_loss, car_index=self._car_index() if self.with_corner_loss else -1,
            sync_cls_avg_factor=_cfg_get(self.train_cfg, 'sync_cls_avg_factor', False),
            sync_reg_avg_factor=_cfg_get(self.train_cfg, 'sync_reg_avg_factor', False))
        self.last_counts = counts
        losses = dict(loss_rcnn_cls=loss_cls, num_pos_rois=num[0], num_neg_rois=num[1], loss_rcnn_bbox=loss_bbox)
        if self.with_corner_loss:
            losses['loss_rcnn_corner'] = loss_corner
        return losses

    def decode_from_rois(self, rois, bbox_pred):
        return roi_decode(rois.contiguous(), _lib.as_fp32(bbox_pred).contiguous(), with_bev=False)[0]

    def get_bboxes_from_tracklet(self, *args, **kwargs):
        raise NotImplementedError('FullySparseBboxHead: get_bboxes_from_tracklet is not built')

    @torch.no_grad()
    def get_bboxes(self, rois, cls_score, bbox_pred, valid_roi_mask, class_labels, class_pred, img_metas, cfg=None):
        """-> per sample (boxes, scores, labels) (:581-684); boxes are wrapped by img_metas[i]['box_type_3d'] when given"""
        assert rois.size(0) == cls_score.size(0) == bbox_pred.size(0)
        assert isinstance(class_labels, list) and isinstance(class_pred, list) and len(class_labels) == len(class_pred) == 1
        cfg = self.test_cfg if cfg is None else cfg
        class_labels, class_pred = list(class_labels), list(class_pred)
        boxes, scores, bev = roi_decode(rois.contiguous(), _lib.as_fp32(bbox_pred).contiguous(),
                                        _lib.as_fp32(cls_score).contiguous())
        if _cfg_get(self.test_cfg, 'rcnn_score_nms', False):
            class_pred[0] = scores
        # regard empty boxes as false positives
        rois, boxes, scores, bev = rois[valid_roi_mask], boxes[valid_roi_mask], scores[valid_roi_mask], bev[valid_roi_mask]
        class_labels[0], class_pred[0] = class_labels[0][valid_roi_mask], class_pred[0][valid_roi_mask]

        def wrap(i, b):
            box_type = (img_metas[i] or {}).get('box_type_3d') if img_metas else None
            return box_type(b, b.size(1)) if box_type is not None else b

        if rois.size(0) == 0:
            return [(wrap(0, boxes), class_pred[0], class_labels[0]), ]
        batch_size = len(class_labels)      # the reference reads roi_batch_id.max(); its own assert above makes it 1
        multi = _cfg_get(cfg, 'multi_class_nms', False) or self.num_classes > 1
        nms_func = self.multi_class_nms if multi else self.single_class_nms
        result_list = []
        for batch_id in range(batch_size):
            selected = nms_func(class_pred[batch_id], class_labels[batch_id], boxes, _cfg_get(cfg, 'score_thr'),
                                _cfg_get(cfg, 'nms_thr'), None, _cfg_get(cfg, 'use_rotate_nms', True), boxes_for_nms=bev)
            if isinstance(selected, list):
                selected = torch.zeros(0, dtype=torch.long, device=boxes.device)
            result_list.append((wrap(batch_id, boxes[selected]), scores[selected], class_labels[batch_id][selected]))
        return result_list

    def multi_class_nms(self, box_probs, labels, box_preds, score_thr, nms_thr, input_meta, use_rotate_nms=True,
                        boxes_for_nms=None):
        """:686-748: per class the score filter and the (rotated) NMS -> the selected indices, class by class"""
        nms_func = box_ops.nms_gpu if use_rotate_nms else box_ops.nms_normal_gpu
        assert box_probs.ndim == 1
        if boxes_for_nms is None:
            boxes_for_nms = box_ops.xywhr2xyxyr(box_ops.lidar_bev(box_preds))
        score_thresh = score_thr if isinstance(score_thr, (list, tuple)) else [score_thr for _ in range(self.num_classes)]
        nms_thresh = nms_thr if isinstance(nms_thr, (list, tuple)) else [nms_thr for _ in range(self.num_classes)]
        selected_list = []
        for k in range(self.num_classes):
            original_idxs = ((box_probs >= score_thresh[k]) & (labels == k)).nonzero(as_tuple=False).view(-1)
            if original_idxs.numel() == 0:
                continue
            cur_selected = nms_func(boxes_for_nms[original_idxs].contiguous(), box_probs[original_idxs], nms_thresh[k])
            if cur_selected.shape[0] == 0:
                continue
            selected_list.append(original_idxs[cur_selected])
        return torch.cat(selected_list, dim=0) if len(selected_list) > 0 else []

    def single_class_nms(self, box_probs, labels, box_preds, score_thr, nms_thr, input_meta, use_rotate_nms=True,
                         boxes_for_nms=None):
        """:750-790"""
        nms_func = box_ops.nms_gpu if use_rotate_nms else box_ops.nms_normal_gpu
        assert box_probs.ndim == 1 and isinstance(score_thr, float)
        if boxes_for_nms is None:
            boxes_for_nms = box_ops.xywhr2xyxyr(box_ops.lidar_bev(box_preds))
        original_idxs = (box_probs >= score_thr).nonzero(as_tuple=False).view(-1)
        if original_idxs.numel() == 0:
            return []
        if nms_thr is None:
            return original_idxs
        cur_selected = nms_func(boxes_for_nms[original_idxs].contiguous(), box_probs[original_idxs], nms_thr)
        return original_idxs[cur_selected] if len(cur_selected) > 0 else []


@HEADS.register_module()
class GroupCorrectionHead(nn.Module):
    """roi_heads/fsd_roi_head.py:14-296: the RoI extractor, the box head, and the fused assignment / sampling around them.
    Built as the cluster heads are: ``build_head(dict(det.unbuilt['roi_head'], train_cfg=det.train_cfg['rcnn'],
    test_cfg=det.test_cfg['rcnn']))``."""

    def __init__(self, num_classes=3, roi_extractor=None, bbox_head=None, train_cfg=None, test_cfg=None, pretrained=None,
                 init_cfg=None):
        super().__init__()
        assert not (init_cfg and pretrained), 'init_cfg and pretrained cannot be setting at the same time'
        self.num_classes = num_classes
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.bbox_head = build_head(dict(bbox_head, train_cfg=train_cfg, test_cfg=test_cfg))
        ext = dict(roi_extractor)
        ext.pop('with_virtual', None)       # the FSDV2 detector's key: it pops it before it builds the head (two_stage_fsd_v2.py:50-53)
        self.roi_extractor = ROI_EXTRACTORS.build(ext)
        self.assign_cfg = self.sample_cfg = None
        if train_cfg:
            class_mask, pos, neg, min_pos = _parse_assigner(train_cfg['assigner'], num_classes)
            self.assign_cfg = dict(class_mask=class_mask, pos_iou_thr=pos, neg_iou_thr=neg, min_pos_iou=min_pos)
            self.sample_cfg = _parse_sampler(train_cfg['sampler'])
            for key in ('class_wise_box_weights', 'class_wise_cls_weights'):
                if _cfg_get(train_cfg, key) is not None:
                    raise NotImplementedError(f'GroupCorrectionHead: train_cfg[\'{key}\'] is not built')

    @property
    def with_bbox(self):
        return True

    def _assign_and_sample(self, proposal_list, gt_bboxes_3d, gt_labels_3d, keys=None, generator=None):
        """-> the dict of ``roi_assign_sample`` (padded rows; ``bbox_head.get_targets`` drops the padding)"""
        assert len(proposal_list) == len(gt_bboxes_3d)
        cfg = self.train_cfg
        return roi_assign_sample([p[0] for p in proposal_list], [p[2] for p in proposal_list], gt_bboxes_3d, gt_labels_3d,
                                 num_classes=self.num_classes, cls_pos_thr=_cfg_get(cfg, 'cls_pos_thr'),
                                 cls_neg_thr=_cfg_get(cfg, 'cls_neg_thr'), keys=keys, generator=generator, **self.assign_cfg,
                                 **self.sample_cfg)

    def _bbox_forward(self, pts_xyz, pts_feats, batch_idx, rois):
        assert pts_xyz.size(0) == pts_feats.size(0) == batch_idx.size(0)
        ext_pts_inds, ext_pts_roi_inds, ext_pts_info = self.roi_extractor(
            pts_xyz[:, :3], batch_idx, rois[:, :8].contiguous(), batch_size=1 if not self.training else None)
        cls_score, bbox_pred, valid_roi_mask = self.bbox_head(pts_xyz[ext_pts_inds], pts_feats[ext_pts_inds], ext_pts_info,
                                                              ext_pts_roi_inds, rois)
        return dict(cls_score=cls_score, bbox_pred=bbox_pred, valid_roi_mask=valid_roi_mask)

    def _bbox_forward_train(self, pts_xyz, pts_feats, batch_idx, sampling_results):
        targets = self.bbox_head.get_targets(sampling_results, self.train_cfg)
        rois = targets['rois']
        bbox_results = self._bbox_forward(pts_xyz, pts_feats, batch_idx, rois)
        bbox_results.update(loss_bbox=self.bbox_head.loss(bbox_results['cls_score'], bbox_results['bbox_pred'],
                                                          bbox_results['valid_roi_mask'], rois, targets))
        return bbox_results

    def forward_train(self, pts_xyz, pts_feats, pts_batch_idx, img_metas, proposal_list, gt_bboxes_3d, gt_labels_3d,
                      keys=None, generator=None):
        """-> the loss dict.  Host reads: ``counts`` (B x 2 integers) and the extractor's own one."""
        sample_results = self._assign_and_sample(proposal_list, gt_bboxes_3d, gt_labels_3d, keys, generator)
        return dict(self._bbox_forward_train(pts_xyz, pts_feats, pts_batch_idx, sample_results)['loss_bbox'])

    @torch.no_grad()
    def simple_test(self, pts_xyz, pts_feats, pts_batch_inds, img_metas, proposal_list, gt_bboxes_3d=None, gt_labels_3d=None,
                    **kwargs):
        """-> per sample (boxes, scores, labels) of ``bbox_head.get_bboxes`` (fsd_roi_head.py:102-160; one sample)"""
        assert len(proposal_list) == 1, 'only support bsz==1 to make cls_preds and labels_3d consistent with bbox_results'
        boxes = [p[0].tensor if hasattr(p[0], 'tensor') else p[0] for p in proposal_list]
        rois = torch.cat([F.pad(b, (1, 0), value=float(i)) for i, b in enumerate(boxes)], dim=0)      # bbox3d2roi
        cls_preds = [res[1] for res in proposal_list]
        labels_3d = [res[2] for res in proposal_list]
        if len(rois) == 0:
            # fake prediction without velocity dims
            rois = torch.tensor([[0, 0, 0, 5, 1, 1, 1, 0]], dtype=rois.dtype).to(rois.device)
            cls_preds = [torch.tensor([0.0], dtype=torch.float32).to(rois.device)]
            labels_3d = [torch.tensor([0], dtype=torch.int64).to(rois.device)]
        bbox_results = self._bbox_forward(pts_xyz, pts_feats, pts_batch_inds, rois)
        return self.bbox_head.get_bboxes(rois, bbox_results['cls_score'], bbox_results['bbox_pred'],
                                         bbox_results['valid_roi_mask'], labels_3d, cls_preds, img_metas, cfg=self.test_cfg)
