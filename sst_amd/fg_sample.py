"""FSD foreground sampling: the stage between the segmentor and the clustering (csrc/fg_sample.hip).

Reference: ``SingleStageFSD.sample`` / ``get_fg_mask`` / ``get_sample_beg_position`` / ``update_sample_results_by_mask`` /
``combine_classes`` (mmdet3d/models/detectors/single_stage_fsd.py:571-593, 698-797).  There the stage is a chain of boolean-mask
indexings - 6 tensors x C classes, each a ``nonzero`` and so a device synchronisation - and it runs again after the cluster
filter.  Here:

``fg_sample_launch`` queues three launches and one memset for all classes and samples: the masks as one 32-bit word per point,
the at-least-one-point rule decided on the device, the row of every selected point (``slot``), the point of every row (``src``)
and the narrow per-class rows (centres, batch index, points) in one concatenated layout.  ``.finish()`` reads ``totals`` and the
rule flags back: the one host read of the stage.  ``fg_sample`` does both and returns the reference's dictionary.

``fg_gather_cat`` replaces the per-class indexing of the wide tensors, their second indexing by the cluster assigner's
``valid_mask`` and the two concatenations by one gather through the composed index; only ``seg_feats`` is differentiable, its
gradient is written row by row in a fixed order (no memset, no float atomic).

There is no eager fall-back: CPU tensors raise."""
import ctypes

import numpy as np
import torch

from . import _lib

WHERE = 'sst_amd.fg_sample'
MAX_CLASSES = 32
STATUS_BAD_BATCH_IDX = 1


def _rows(where, t, cols, what):
    """a 2-D float32 device tensor whose rows are dense (any row stride) with at least ``cols`` columns -> its row stride"""
    check_f32_strided(where, t)
    if t.dim() != 2 or t.size(1) < cols or (t.size(1) > 1 and t.stride(1) != 1):
        raise RuntimeError(f'{where}: {what} must be [N, >= {cols}] with unit column stride, got {tuple(t.shape)} '
                           f'strides {t.stride()}')
    return t.stride(0) if t.size(0) > 1 else max(t.stride(0), t.size(1))


def check_f32_strided(where, t):
    if not t.is_cuda:
        raise RuntimeError('sst_amd: tensor must be a CUDA/HIP tensor (no CPU path in this library)')
    if t.dtype != torch.float32:
        raise RuntimeError(f'{where}: float32 tensors expected, got {t.dtype}')


def round_thresholds(score_thresh, threshold_buffer=0.0):
    """``score_thresh[c] + threshold_buffer`` in Python's double, then rounded to float32 once: what torch does with a Python
    scalar operand of a float32 comparison (single_stage_fsd.py:771)"""
    return [float(np.float32(float(t) + float(threshold_buffer))) for t in score_thresh]


class FgSamplePending(object):
    """what ``fg_sample_launch`` queued; ``finish()`` reads the totals (one host read) and cuts the per-class views"""

    def __init__(self, n, num_classes, batch_idx, point_cols, dev, max_rows=None, aux_rows=None):
        self.n, self.num_classes = n, num_classes
        c, rows = num_classes, num_classes * n if max_rows is None else int(max_rows)
        self.max_rows = rows
        if aux_rows is not None:
            self.aux_out = torch.empty(rows, dtype=torch.int32, device=dev)
            self.aux_inv = torch.empty(int(aux_rows), dtype=torch.int32, device=dev)
        self.slot = torch.empty((c, n), dtype=torch.int32, device=dev)
        self.mask = torch.empty((c, n), dtype=torch.bool, device=dev)
        self.src = torch.empty(rows, dtype=torch.int32, device=dev)
        self.centers = torch.empty((rows, 3), dtype=torch.float32, device=dev)
        self.batch_out = torch.empty(rows, dtype=batch_idx.dtype, device=dev)
        self.points_out = torch.empty((rows, point_cols), dtype=torch.float32, device=dev)
        self.info = torch.zeros(3 * c + 2, dtype=torch.int32, device=dev) if n == 0 else \
            torch.empty(3 * c + 2, dtype=torch.int32, device=dev)
        self._result = None

    def finish(self):
        if self._result is not None:
            return self._result
        c = self.num_classes
        info = self.info.tolist() if self.n > 0 else [0] * (3 * c + 2)       # the one host read of the stage
        if info[3 * c + 1] & STATUS_BAD_BATCH_IDX:
            raise RuntimeError(f'{WHERE}: batch_idx holds a value outside [0, batch_size)')
        totals, rule, off = info[:c], [bool(r) for r in info[c:2 * c]], info[2 * c:3 * c + 1]
        cut = lambda t: [t[off[k]:off[k + 1]] for k in range(c)]
        self._result = dict(seg_points=cut(self.points_out), batch_idx=cut(self.batch_out), center_preds=cut(self.centers),
                            fg_mask_list=list(self.mask.unbind(0)), src=cut(self.src), src_cat=self.src[:off[c]],
                            center_cat=self.centers[:off[c]], points_cat=self.points_out[:off[c]], batch_cat=self.batch_out[:off[c]],
                            slot=self.slot, class_offsets=off, totals=totals, rule=rule)
        return self._result


def fg_sample_launch(seg_logits, vote_offsets, seg_points, batch_idx, thresholds, batch_size, extra_mask=None,
                     apply_rule=True, validate=False, sample_major=False, aux=None, aux_rows=0, max_rows=None):
    """Queue the sampling of all classes (no host read) -> FgSamplePending.

    seg_logits [N, C] fp32 (any row stride) or None (``extra_mask`` alone decides); vote_offsets [N, 3C]; seg_points [N, P >= 3];
    batch_idx [N] int32 / int64, NON-DECREASING (what ``voxelize_batch`` and ``pre_voxelize`` give; ``validate=True`` checks it
    with one torch comparison, a host read); thresholds: C floats, already rounded (``round_thresholds``), +inf disables the
    compare of a class; extra_mask: bool [C, N] ORed in (top-k indices, points in ground-truth boxes); batch_size: samples.

    ``sample_major`` (what ``roi_input`` uses): ONE output layout sorted by sample and, inside a sample, class after class;
    ``slot`` then holds the output row, ``aux`` int32 [C, N] rides along (``aux_out``, and ``aux_inv`` [aux_rows] its
    inverse) and ``max_rows`` bounds the rows that are written."""
    c = len(thresholds)
    if c < 1 or c > MAX_CLASSES:
        raise NotImplementedError(f'{WHERE}: {c} classes; the mask word holds 1 to {MAX_CLASSES} (SST_FG_MAX_CLASSES)')
    if batch_size < 1:
        raise RuntimeError(f'{WHERE}: batch_size must be positive, got {batch_size}')
    ld_p = _rows(WHERE, seg_points, 3, 'seg_points')
    n, dev = seg_points.size(0), seg_points.device
    ld_l = ld_v = 0
    if seg_logits is not None:
        ld_l = _rows(WHERE, seg_logits, c, 'seg_logits')
        if seg_logits.size(1) != c or seg_logits.size(0) != n:
            raise RuntimeError(f'{WHERE}: seg_logits must be [{n}, {c}], got {tuple(seg_logits.shape)}')
    elif extra_mask is None:
        raise RuntimeError(f'{WHERE}: neither seg_logits nor extra_mask')
    if vote_offsets is not None:
        ld_v = _rows(WHERE, vote_offsets, 3 * c, 'vote_offsets')
        if vote_offsets.size(0) != n:
            raise RuntimeError(f'{WHERE}: vote_offsets must have {n} rows, got {vote_offsets.size(0)}')
    if batch_idx.is_cuda and not batch_idx.is_contiguous():      # a column of the voxel coordinates (pre_voxelize): a narrow copy
        batch_idx = batch_idx.contiguous()
    _lib.require_cuda(batch_idx, extra_mask)
    if batch_idx.dtype not in (torch.int32, torch.int64) or tuple(batch_idx.shape) != (n,):
        raise RuntimeError(f'{WHERE}: batch_idx must be int32 / int64 of shape ({n},), got {batch_idx.dtype} '
                           f'{tuple(batch_idx.shape)}')
    if extra_mask is not None and (extra_mask.dtype != torch.bool or tuple(extra_mask.shape) != (c, n)):
        raise RuntimeError(f'{WHERE}: extra_mask must be bool of shape ({c}, {n}), got {extra_mask.dtype} '
                           f'{tuple(extra_mask.shape)}')
    if validate and n > 1 and bool((batch_idx[1:] < batch_idx[:-1]).any()):
        raise RuntimeError(f'{WHERE}: batch_idx must be non-decreasing')
    if aux is not None and (aux.dtype != torch.int32 or tuple(aux.shape) != (c, n) or not aux.is_cuda or not aux.is_contiguous()):
        raise RuntimeError(f'{WHERE}: aux must be a contiguous device int32 tensor of shape ({c}, {n})')
    pend = FgSamplePending(n, c, batch_idx, seg_points.size(1), dev, max_rows, aux_rows if aux is not None else None)
    if n == 0:
        return pend
    lib = _lib.load()
    a = _lib.FgSampleArgs()
    a.logits, a.votes, a.points = _lib.ptr(seg_logits), _lib.ptr(vote_offsets), _lib.ptr(seg_points)
    a.batch_idx, a.extra_mask = _lib.ptr(batch_idx), _lib.ptr(extra_mask)
    a.slot, a.mask, a.src, a.info = _lib.ptr(pend.slot), _lib.ptr(pend.mask), _lib.ptr(pend.src), _lib.ptr(pend.info)
    a.centers = _lib.ptr(pend.centers) if vote_offsets is not None else None
    a.batch_out, a.points_out = _lib.ptr(pend.batch_out), _lib.ptr(pend.points_out)
    a.n, a.ld_logits, a.ld_votes, a.ld_points = n, ld_l, ld_v, ld_p
    a.num_classes, a.point_cols, a.batch = c, seg_points.size(1), int(batch_size)
    a.batch_is_i64, a.apply_rule = int(batch_idx.dtype == torch.int64), int(bool(apply_rule))
    a.sample_major, a.max_rows = int(bool(sample_major)), pend.max_rows
    if aux is not None:
        a.aux, a.aux_out, a.aux_inv, a.aux_rows = _lib.ptr(aux), _lib.ptr(pend.aux_out), _lib.ptr(pend.aux_inv), int(aux_rows)
    for k, t in enumerate(thresholds):
        a.thresholds[k] = float(t)
    ws = _lib.workspace(lib.sst_fg_sample_workspace_bytes(n, c, int(batch_size)), dev)
    _lib.check(lib.sst_fg_sample_f32(ctypes.byref(a), _lib.ptr(ws), _lib.stream_ptr()), 'sst_fg_sample_f32')
    return pend


def fg_sample(seg_logits, vote_offsets, seg_points, batch_idx, thresholds, batch_size, extra_mask=None, apply_rule=True,
              validate=False):
    """-> the reference's ``sample`` dictionary as lists per class (``seg_points``, ``batch_idx``, ``center_preds``,
    ``fg_mask_list``) plus ``src`` (the point of every row), ``slot`` [C, N] (the row of every point, -1), ``class_offsets``,
    ``totals`` and ``rule`` (did the at-least-one-point rule fire for the class)"""
    return fg_sample_launch(seg_logits, vote_offsets, seg_points, batch_idx, thresholds, batch_size, extra_mask, apply_rule,
                            validate).finish()


def topk_extra_mask(seg_logits, topks, classes=None):
    """the ``disable_pretrain`` state of get_fg_mask (:757-763): per class the indices of ``torch.topk`` of the scores, set in a
    bool [C, N] (rows of classes outside ``classes`` stay False).  The sigmoid is monotonic, but the reference ranks the scores:
    so does this."""
    n, c = seg_logits.shape
    mask = torch.zeros((c, n), dtype=torch.bool, device=seg_logits.device)
    scores = seg_logits.sigmoid()
    for k in (range(c) if classes is None else classes):
        mask[k, torch.topk(scores[:, k], min(int(topks[k]), n))[1]] = True
    return mask


def gt_extra_mask(seg_points, batch_idx, gt_bboxes_3d, gt_labels_3d, num_classes, out=None):
    """``add_gt_fg_points`` (:776-794): bool [C, N], True where a point lies in a ground-truth box of that class of its own sample.
    No host read: every sample's boxes are tested against all points and the answer kept where ``batch_idx`` names the sample;
    the boxes of other classes are replaced by an empty box far away instead of being indexed out."""
    from . import box_ops
    n, dev = seg_points.size(0), seg_points.device
    mask = out if out is not None else torch.zeros((num_classes, n), dtype=torch.bool, device=dev)
    if n == 0:
        return mask
    xyz = seg_points[:, :3].contiguous()[None]
    far = torch.tensor([1e30, 1e30, 1e30, 0., 0., 0., 0.], dtype=torch.float32, device=dev)
    for s, (boxes, labels) in enumerate(zip(gt_bboxes_3d, gt_labels_3d)):
        boxes = getattr(boxes, 'tensor', boxes)
        if boxes.size(0) == 0:
            continue
        boxes = boxes[:, :7].to(dev, torch.float32)
        mine = batch_idx == s
        for k in range(num_classes):
            sel = torch.where((labels.to(dev) == k)[:, None], boxes, far[None])
            mask[k] |= (box_ops.points_in_boxes_gpu(xyz, sel[None].contiguous())[0] > -1) & mine
    return mask


class _GatherCat(torch.autograd.Function):

    @staticmethod
    def forward(ctx, seg_feats, seg_logits, seg_vote_preds, seg_points, idx, slot2):
        m, dev = idx.numel(), seg_feats.device
        cl, cv, cf, cp = seg_logits.size(1), seg_vote_preds.size(1), seg_feats.size(1), seg_points.size(1)
        out = torch.empty((m, cl + cv + cf), dtype=torch.float32, device=dev)
        pts = torch.empty((m, cp), dtype=torch.float32, device=dev)
        if m > 0:
            g = _lib.FgGatherArgs()
            g.idx, g.out, g.points_out = _lib.ptr(idx), _lib.ptr(out), _lib.ptr(pts)
            g.logits, g.votes, g.feats, g.points = (_lib.ptr(t) for t in (seg_logits, seg_vote_preds, seg_feats, seg_points))
            g.ld_logits, g.ld_votes = _rows(WHERE, seg_logits, cl, 'seg_logits'), _rows(WHERE, seg_vote_preds, cv, 'seg_vote_preds')
            g.ld_feats, g.ld_points = _rows(WHERE, seg_feats, cf, 'seg_feats'), _rows(WHERE, seg_points, cp, 'seg_points')
            g.m, g.n, g.c_logits, g.c_votes, g.c_feats, g.c_points = m, seg_feats.size(0), cl, cv, cf, cp
            _lib.check(_lib.load().sst_fg_gather_cat_fwd_f32(ctypes.byref(g), _lib.stream_ptr()), 'sst_fg_gather_cat_fwd_f32')
        ctx.save_for_backward(slot2)
        ctx.shape = (seg_feats.size(0), cf, cl + cv)
        ctx.mark_non_differentiable(pts)
        return out, pts

    @staticmethod
    def backward(ctx, d_out, _d_pts):
        slot2, = ctx.saved_tensors
        n, cf, col0 = ctx.shape
        d_out = d_out.contiguous()
        d_feats = torch.empty((n, cf), dtype=torch.float32, device=d_out.device)
        _lib.check(_lib.load().sst_fg_gather_cat_bwd_f32(_lib.ptr(d_out), d_out.size(0), d_out.size(1), col0, _lib.ptr(slot2), n,
                                                         slot2.size(0),
                                                         cf, _lib.ptr(d_feats), _lib.stream_ptr()), 'sst_fg_gather_cat_bwd_f32')
        return d_feats, None, None, None, None, None


def final_slots(slot, keep_list):
    """update_sample_results_by_mask for the masks (:575-582), one launch: ``keep_list[c]``: int64 rows of class c that pass the
    cluster filter, ascending (``valid_mask._sst_keep``) -> (slot2 int32 [C, N]: the row in the combined output or -1,
    final masks bool [C, N] = the reference's ``new_data[data] = mask``)"""
    c, n = slot.shape
    if len(keep_list) != c:
        raise RuntimeError(f'{WHERE}: {len(keep_list)} keep lists for {c} classes')
    _lib.require_cuda(slot, *keep_list)
    keep = torch.cat([k.to(torch.int64) for k in keep_list]) if c > 1 else keep_list[0].to(torch.int64).contiguous()
    off = [0]
    for k in keep_list:
        off.append(off[-1] + k.numel())
    slot2 = torch.empty((c, n), dtype=torch.int32, device=slot.device)
    fmask = torch.empty((c, n), dtype=torch.bool, device=slot.device)
    _lib.check(_lib.load().sst_fg_slot2_i32(_lib.ptr(slot), n, c, _lib.ptr(keep), _lib.i64array(off), _lib.ptr(slot2),
                                            _lib.ptr(fmask), _lib.stream_ptr()), 'sst_fg_slot2_i32')
    return slot2, fmask


def keep_of(valid_mask):
    """the rows a cluster assigner's ``valid_mask`` keeps: the index list the assigners attach (``_sst_keep``, no search), else
    ``nonzero`` (a host read: masks from elsewhere)"""
    keep = getattr(valid_mask, '_sst_keep', None)
    return keep if keep is not None else torch.nonzero(valid_mask)[:, 0]


def fg_gather_cat(sampled, valid_mask_list, seg_logits, seg_vote_preds, seg_feats, seg_points, detach_feats=False):
    """The data flow of single_stage_fsd.py:527-532 after the cluster filter, as one gather: ``sampled`` is ``fg_sample``'s
    result, ``valid_mask_list`` the assigner's masks over each class's rows (or index lists).
    -> dict(pts_feats [M, C + 3C + F] = cat(seg_logits, seg_vote_preds, seg_feats)[idx], seg_points [M, P], center_preds [M, 3],
    fg_mask_list (final masks per class), idx int32 [M], slot2 int32 [C, N]).  seg_logits and seg_vote_preds are detached, as in
    the reference (:510-511); seg_feats receives the gradient unless ``detach_feats`` (``train_cfg.detach_segmentor``)."""
    check_f32_strided(WHERE, seg_feats)
    keeps = [v if v.dtype != torch.bool else keep_of(v) for v in valid_mask_list]
    slot2, fmask = final_slots(sampled['slot'], keeps)
    idx = torch.cat([s[k] for s, k in zip(sampled['src'], keeps)])
    centers = torch.cat([t[k] for t, k in zip(sampled['center_preds'], keeps)])
    feats = seg_feats.detach() if detach_feats else seg_feats
    out, pts = _GatherCat.apply(feats, seg_logits.detach(), seg_vote_preds.detach(), seg_points.detach(), idx, slot2)
    return dict(pts_feats=out, seg_points=pts, center_preds=centers, fg_mask_list=list(fmask.unbind(0)), idx=idx, slot2=slot2)


def slots_of_masks(masks):
    """bool [C, N] -> int32 [C, N]: the row of (class, point) in the class-after-class concatenation of the selected points,
    -1 where the mask is False (``slot2`` of ``fg_gather_cat`` restated from its final masks; a cumulative sum, no host read)"""
    flat = masks.reshape(-1)
    rows = torch.cumsum(flat, 0, dtype=torch.int32) - 1
    return torch.where(flat, rows, torch.full_like(rows, -1)).view(masks.shape)


class _RoiCat(torch.autograd.Function):

    @staticmethod
    def forward(ctx, cluster_feats, seg_feats, src, row, inv, dest, rows):
        fc, f = cluster_feats.size(1), seg_feats.size(1)
        out = torch.empty((rows, fc + f), dtype=torch.float32, device=seg_feats.device)
        ld_c = _rows(WHERE, cluster_feats, fc, 'cluster_pts_feats') if cluster_feats.size(0) > 0 else fc
        ld_f = _rows(WHERE, seg_feats, f, 'seg_feats') if seg_feats.size(0) > 0 else f
        _lib.check(_lib.load().sst_fg_roi_cat_fwd_f32(_lib.ptr(src), _lib.ptr(row), rows, seg_feats.size(0), cluster_feats.size(0),
                                                      _lib.ptr(cluster_feats), ld_c, fc,
                                                      _lib.ptr(seg_feats), ld_f, f, _lib.ptr(out), _lib.stream_ptr()),
                   'sst_fg_roi_cat_fwd_f32')
        ctx.save_for_backward(inv, dest)
        ctx.dims = (cluster_feats.size(0), fc, seg_feats.size(0), f)
        return out

    @staticmethod
    def backward(ctx, d_out):
        inv, dest = ctx.saved_tensors
        m, fc, n, f = ctx.dims
        d_out = d_out.contiguous()
        lib, d_cluster, d_seg = _lib.load(), None, None
        if ctx.needs_input_grad[0]:                      # a row read: the first fc columns of the row each cluster row went to
            d_cluster = torch.empty((m, fc), dtype=torch.float32, device=d_out.device)
            g = _lib.FgGatherArgs()
            g.idx, g.feats, g.out = _lib.ptr(inv), _lib.ptr(d_out), _lib.ptr(d_cluster)
            g.m, g.n, g.ld_feats, g.c_feats = m, d_out.size(0), d_out.size(1), fc
            _lib.check(lib.sst_fg_gather_cat_fwd_f32(ctypes.byref(g), _lib.stream_ptr()), 'sst_fg_gather_cat_fwd_f32')
        if ctx.needs_input_grad[1]:                      # the point's copies in the fixed order: background, then each class
            d_seg = torch.empty((n, f), dtype=torch.float32, device=d_out.device)
            _lib.check(lib.sst_fg_gather_cat_bwd_f32(_lib.ptr(d_out), d_out.size(0), d_out.size(1), fc, _lib.ptr(dest), n,
                                                     dest.size(0), f,
                                                     _lib.ptr(d_seg), _lib.stream_ptr()), 'sst_fg_gather_cat_bwd_f32')
        return d_cluster, d_seg, None, None, None, None, None


def _stack_masks(pts_mask):
    masks = torch.stack(list(pts_mask)) if isinstance(pts_mask, (list, tuple)) else pts_mask
    if not masks.is_cuda:
        raise RuntimeError('sst_amd: tensor must be a CUDA/HIP tensor (no CPU path in this library)')
    if masks.dtype != torch.bool or masks.dim() != 2:
        raise RuntimeError(f'{WHERE}: the masks must be bool [C, N], got {masks.dtype} {tuple(masks.shape)}')
    return masks.contiguous()


def roi_input(points, cluster_pts_feats, seg_feats, pts_mask, batch_idx, batch_size, slot2=None, num_rows=None,
              detach_seg_feats=False, detach_cluster_feats=False):
    """``FSD.prepare_multi_class_roi_input`` (mmdet3d/models/detectors/two_stage_fsd.py:127-178) -> (all_points [R, P],
    cat_feats [R, Fc + F], all_batch_inds [R], pending).

    ``pts_mask``: the final masks per class (list or bool [C, N]); ``cluster_pts_feats`` [M, Fc]: the rows of the selected points
    class after class (``slot2`` int32 [C, N], when the caller has it, names the row of every (class, point); else it is
    restated from the masks).  The rows are sorted by sample; inside a sample: the background points (no mask set) in point
    order, then the points of class 0, class 1, ...: the STABLE sort of the reference's concatenation (the reference calls
    ``Tensor.sort()`` without ``stable``, which leaves the order inside a sample open on a GPU).  ``num_rows`` = R (background
    points + M) when the caller knows it: then nothing is read back; else one read of the totals.  The reference's ``isclose``
    assert on the points (a device read) is dropped."""
    masks = _stack_masks(pts_mask)
    c, n = masks.shape
    if c + 1 > MAX_CLASSES:
        raise NotImplementedError(f'{WHERE}: roi_input with {c} classes; the background takes one of the {MAX_CLASSES} mask bits')
    check_f32_strided(WHERE, cluster_pts_feats)
    check_f32_strided(WHERE, seg_feats)
    m = cluster_pts_feats.size(0)
    if slot2 is None:
        slot2 = slots_of_masks(masks)
    ext = torch.cat([~masks.any(0, keepdim=True), masks])                       # pseudo-class 0: the background
    aux = torch.cat([torch.full_like(slot2[:1], -1), slot2]).contiguous()
    alloc = int(num_rows) if num_rows is not None else n + m
    pend = fg_sample_launch(None, None, points, batch_idx, [float('inf')] * (c + 1), batch_size, extra_mask=ext,
                            apply_rule=False, sample_major=True, aux=aux, aux_rows=m, max_rows=alloc)
    rows = alloc
    if num_rows is None and n > 0:
        rows = pend.finish()['class_offsets'][c + 1]
    if n == 0:
        rows = 0
    if detach_seg_feats:
        seg_feats = seg_feats.detach()
    if detach_cluster_feats:
        cluster_pts_feats = cluster_pts_feats.detach()
    cat_feats = _RoiCat.apply(cluster_pts_feats, seg_feats, pend.src, getattr(pend, 'aux_out', None), getattr(pend, 'aux_inv', None),
                              pend.slot, rows)
    return pend.points_out[:rows], cat_feats, pend.batch_out[:rows], pend


def roi_input_single(points, cluster_pts_feats, seg_feats, pts_mask, batch_idx, slot2=None, detach_seg_feats=False,
                     detach_cluster_feats=False):
    """``FSD.prepare_roi_input`` (two_stage_fsd.py:108-125), the single-class form: the cluster features padded in place with
    zeros, no reordering -> (points, cat_feats [N, Fc + F], batch_idx).  No host read."""
    masks = _stack_masks(pts_mask)
    if masks.size(0) != 1:
        raise RuntimeError(f'{WHERE}: prepare_roi_input is the single-class form, got {masks.size(0)} masks')
    check_f32_strided(WHERE, cluster_pts_feats)
    check_f32_strided(WHERE, seg_feats)
    n, m = masks.size(1), cluster_pts_feats.size(0)
    if slot2 is None:
        slot2 = slots_of_masks(masks)
    row = slot2[0].contiguous()
    point_of = torch.empty(m + 1, dtype=torch.int32, device=masks.device)       # the inverse of row; slot m takes the rest
    point_of[torch.where(row >= 0, row, torch.full_like(row, m)).long()] = torch.arange(n, dtype=torch.int32, device=masks.device)
    dest = torch.arange(n, dtype=torch.int32, device=masks.device)[None]
    if detach_seg_feats:
        seg_feats = seg_feats.detach()
    if detach_cluster_feats:
        cluster_pts_feats = cluster_pts_feats.detach()
    cat_feats = _RoiCat.apply(cluster_pts_feats, seg_feats, None, row, point_of[:m], dest, n)
    return points, cat_feats, batch_idx
