"""FSDv2 grouped foreground sampling: the stage between the segmentor and the virtual voxels (csrc/fg_group_sample.hip,
DESIGN.md 3.19).

Reference: ``SingleStageFSDV2.batched_group_sample`` / ``group_sample`` with ``get_fg_mask``, ``gather_group_by_names``,
``get_sample_beg_position`` and ``get_offset_weight`` (mmdet3d/models/detectors/single_stage_fsd_v2.py:656-705, 726-891), and the
projector input of ``extract_feat`` (:164-176).  There the stage is a softmax, a column gather and a sum per group, then a chain
of boolean-mask indexings - 6 tensors x G groups, each a ``nonzero`` and so a device synchronisation - plus ``unique`` /
``.item()`` decisions.  Here:

``group_sample_launch`` queues three launches and one memset for all groups and samples: the softmax scores summed per group and
compared, the masks as one 32-bit word per point, the at-least-one-point rule decided on the device, the row of every selected
point (``slot``), the point of every row (``src``) and the narrow rows (voted centres with the ``'max'`` offset weights, batch
index, points) in the layout of ``fg_sample``.  ``.finish()`` reads the totals and rule flags back: the one host read.

``virtual_rows`` writes the projector's input ``cat(seg_feats, (clip(centre) - xyz) / 10, seg_logits, points[:, 3:])`` of the
sampled rows in one gather and returns the clipped centres; only ``seg_feats`` is differentiable, its gradient is written row by
row in a fixed order (no memset, no float atomic).  It serves the per-class path (rows from ``fg_sample``) as well.  The rows
equal ``extract_feat``'s own concatenation on the device bit for bit: the division by 10 is, as torch's for a device tensor and a
scalar, a product with the float32 reciprocal.

There is no eager fall-back: CPU tensors raise."""
import ctypes

import torch

from . import _lib
from .fg_sample import FgSamplePending, _rows, check_f32_strided, round_thresholds  # noqa: F401

WHERE = 'sst_amd.fg_group_sample'
MAX_GROUPS = 32
MAX_LOGITS = 64


def groups_by_names(group_names, class_names):
    """``group_names`` (lists of class names) -> lists of class indices, as gather_group_by_names (:879-888) looks them up; a
    name missing from ``class_names`` is refused by name"""
    groups = []
    for names in group_names:
        for name in names:
            if name not in class_names:
                raise NotImplementedError(f'{WHERE}: group class {name!r} is missing from class_names {list(class_names)}')
        groups.append([list(class_names).index(name) for name in names])
    return groups


def check_groups(groups, num_logits):
    """the refusals by name: G > 32, K > 64, a class listed in two groups (or twice), an index that is not a foreground column"""
    g = len(groups)
    if g < 1 or g > MAX_GROUPS:
        raise NotImplementedError(f'{WHERE}: {g} groups; the mask word holds 1 to {MAX_GROUPS} (SST_FG_MAX_CLASSES)')
    if num_logits > MAX_LOGITS:
        raise NotImplementedError(f'{WHERE}: {num_logits} logit columns; the kernel takes up to {MAX_LOGITS} (SST_FG_MAX_LOGITS)')
    seen = {}
    for gi, grp in enumerate(groups):
        if len(grp) == 0:
            raise NotImplementedError(f'{WHERE}: group {gi} lists no class')
        for k in grp:
            k = int(k)
            if k < 0 or k >= num_logits - 1:
                raise NotImplementedError(f'{WHERE}: group {gi} lists class {k}; the foreground columns are 0 .. {num_logits - 2} '
                                          f'(the last of the {num_logits} logits is the background, never part of a group)')
            if k in seen:
                raise NotImplementedError(f'{WHERE}: class {k} is listed in two groups ({seen[k]} and {gi}); the kernel reads each '
                                          'class in one group')
            seen[k] = gi
    return [[int(k) for k in grp] for grp in groups]


def group_sample_launch(seg_logits, vote_offsets, seg_points, batch_idx, groups, thresholds, batch_size, offset_scale=1,
                        extra_mask=None, apply_rule=True, validate=False):
    """Queue the sampling of all groups (no host read) -> FgSamplePending.

    seg_logits [N, K = C + 1] fp32 (any row stride), the background last; vote_offsets [N, 3K]; seg_points [N, P >= 3]; batch_idx
    [N] int32 / int64, NON-DECREASING (``validate=True`` checks it with one torch comparison, a host read); groups: G lists of
    class indices; thresholds: G floats, already rounded (``round_thresholds``), +inf disables the compare of a group; extra_mask:
    bool [G, N] ORed in (``group_topk_extra_mask``); batch_size: samples; offset_scale: ``cfg['offset_scale']`` (:810)."""
    if seg_logits.dim() != 2:
        raise RuntimeError(f'{WHERE}: seg_logits must be [N, K], got {tuple(seg_logits.shape)}')
    n, k = seg_logits.shape
    groups = check_groups(groups, k)                     # the refusals by name come first: they do not depend on the device
    check_f32_strided(WHERE, seg_logits)
    g = len(groups)
    if len(thresholds) != g:
        raise RuntimeError(f'{WHERE}: {len(thresholds)} thresholds for {g} groups')
    if batch_size < 1:
        raise RuntimeError(f'{WHERE}: batch_size must be positive, got {batch_size}')
    ld_p = _rows(WHERE, seg_points, 3, 'seg_points')
    ld_l = _rows(WHERE, seg_logits, k, 'seg_logits')
    ld_v = _rows(WHERE, vote_offsets, 3 * k, 'vote_offsets')
    dev = seg_points.device
    if seg_points.size(0) != n or vote_offsets.size(0) != n or vote_offsets.size(1) != 3 * k:
        raise RuntimeError(f'{WHERE}: seg_points must have {n} rows and vote_offsets be [{n}, {3 * k}], got '
                           f'{tuple(seg_points.shape)} and {tuple(vote_offsets.shape)}')
    if batch_idx.is_cuda and not batch_idx.is_contiguous():
        batch_idx = batch_idx.contiguous()
    _lib.require_cuda(batch_idx, extra_mask)
    if batch_idx.dtype not in (torch.int32, torch.int64) or tuple(batch_idx.shape) != (n,):
        raise RuntimeError(f'{WHERE}: batch_idx must be int32 / int64 of shape ({n},), got {batch_idx.dtype} '
                           f'{tuple(batch_idx.shape)}')
    if extra_mask is not None and (extra_mask.dtype != torch.bool or tuple(extra_mask.shape) != (g, n)):
        raise RuntimeError(f'{WHERE}: extra_mask must be bool of shape ({g}, {n}), got {extra_mask.dtype} '
                           f'{tuple(extra_mask.shape)}')
    if validate and n > 1 and bool((batch_idx[1:] < batch_idx[:-1]).any()):
        raise RuntimeError(f'{WHERE}: batch_idx must be non-decreasing')
    pend = FgSamplePending(n, g, batch_idx, seg_points.size(1), dev)
    if n == 0:
        return pend
    lib = _lib.load()
    a = _lib.FgGroupSampleArgs()
    a.logits, a.votes, a.points = _lib.ptr(seg_logits), _lib.ptr(vote_offsets), _lib.ptr(seg_points)
    a.batch_idx, a.extra_mask = _lib.ptr(batch_idx), _lib.ptr(extra_mask)
    a.slot, a.mask, a.src, a.info = _lib.ptr(pend.slot), _lib.ptr(pend.mask), _lib.ptr(pend.src), _lib.ptr(pend.info)
    a.centers, a.batch_out, a.points_out = _lib.ptr(pend.centers), _lib.ptr(pend.batch_out), _lib.ptr(pend.points_out)
    a.n, a.ld_logits, a.ld_votes, a.ld_points, a.max_rows = n, ld_l, ld_v, ld_p, pend.max_rows
    a.num_groups, a.num_logits, a.point_cols, a.batch = g, k, seg_points.size(1), int(batch_size)
    a.batch_is_i64, a.apply_rule = int(batch_idx.dtype == torch.int64), int(bool(apply_rule))
    a.offset_scale = float(offset_scale)                 # ctypes rounds the double to float32 once, as torch does the scalar
    pos = 0
    for gi, grp in enumerate(groups):
        a.thresholds[gi] = float(thresholds[gi])
        a.group_begin[gi] = pos
        for c in grp:
            a.group_class[pos] = c
            pos += 1
    a.group_begin[g] = pos
    ws = _lib.workspace(lib.sst_fg_group_sample_workspace_bytes(n, g, int(batch_size)), dev)
    _lib.check(lib.sst_fg_group_sample_f32(ctypes.byref(a), _lib.ptr(ws), _lib.stream_ptr()), 'sst_fg_group_sample_f32')
    return pend


def group_sample(seg_logits, vote_offsets, seg_points, batch_idx, groups, thresholds, batch_size, offset_scale=1, extra_mask=None,
                 apply_rule=True, validate=False):
    """-> the reference's ``batched_group_sample`` dictionary as lists per group (``seg_points``, ``batch_idx``, ``center_preds``,
    ``fg_mask_list``) plus ``src`` (the point of every row), ``src_cat``, ``slot`` [G, N] (the row of every point inside its
    group, -1), ``class_offsets``, ``totals`` and ``rule`` (did the at-least-one-point rule fire for the group)"""
    return group_sample_launch(seg_logits, vote_offsets, seg_points, batch_idx, groups, thresholds, batch_size, offset_scale,
                               extra_mask, apply_rule, validate).finish()


def grouped_scores(seg_logits, groups):
    """gather_group_by_names (:879-891) over ``seg_logits.softmax(1)`` -> [N, G]"""
    scores = seg_logits.softmax(1)
    return torch.stack([scores[:, list(grp)].sum(1) for grp in groups], dim=1)


def group_topk_extra_mask(seg_logits, groups, topks):
    """the ``disable_pretrain`` state of get_fg_mask (:663-669) on the grouped path: per group the indices of ``torch.topk`` of
    the grouped softmax scores, set in a bool [G, N]"""
    if not seg_logits.is_cuda:
        raise RuntimeError('sst_amd: tensor must be a CUDA/HIP tensor (no CPU path in this library)')
    n = seg_logits.size(0)
    groups = check_groups(groups, seg_logits.size(1))
    scores = grouped_scores(seg_logits, groups)
    mask = torch.zeros((len(groups), n), dtype=torch.bool, device=seg_logits.device)
    for gi in range(len(groups)):
        mask[gi, torch.topk(scores[:, gi], min(int(topks[gi]), n))[1]] = True
    return mask


def clip_bounds(pc_range, eps=1e-5):
    """the float32 bounds of ``VirtualVoxelExtractor.clip_points``: the float32 range plus / minus eps in float32 arithmetic,
    formed on the host (the same two tensor operations on the CPU) -> (lo, hi) lists of 3 floats"""
    r = torch.tensor([float(v) for v in pc_range], dtype=torch.float32)
    return (r[:3] + eps).tolist(), (r[3:] - eps).tolist()


class _VirtualRows(torch.autograd.Function):

    @staticmethod
    def forward(ctx, seg_feats, seg_logits, seg_points, centers, src, slot, offsets, lo, hi):
        m, n = src.numel(), seg_feats.size(0)
        cf, cl, cp = seg_feats.size(1), seg_logits.size(1), seg_points.size(1)
        out = torch.empty((m, cf + 3 + cl + cp - 3), dtype=torch.float32, device=seg_feats.device)
        clipped = torch.empty((m, 3), dtype=torch.float32, device=seg_feats.device)
        if m > 0:
            v = _lib.FgVirtualRowsArgs()
            v.src, v.centers, v.out, v.clipped = _lib.ptr(src), _lib.ptr(centers), _lib.ptr(out), _lib.ptr(clipped)
            v.feats, v.logits, v.points = _lib.ptr(seg_feats), _lib.ptr(seg_logits), _lib.ptr(seg_points)
            v.ld_feats, v.ld_logits = _rows(WHERE, seg_feats, cf, 'seg_feats'), _rows(WHERE, seg_logits, cl, 'seg_logits')
            v.ld_points = _rows(WHERE, seg_points, cp, 'seg_points')
            v.m, v.n, v.c_feats, v.c_logits, v.c_points = m, n, cf, cl, cp
            for k in range(3):
                v.lo[k], v.hi[k] = lo[k], hi[k]
            _lib.check(_lib.load().sst_fg_virtual_rows_fwd_f32(ctypes.byref(v), _lib.stream_ptr()), 'sst_fg_virtual_rows_fwd_f32')
        ctx.save_for_backward(slot)
        ctx.meta = (n, cf, tuple(offsets))
        ctx.mark_non_differentiable(clipped)
        return out, clipped

    @staticmethod
    def backward(ctx, d_out, _d_clipped):
        slot, = ctx.saved_tensors
        n, cf, offsets = ctx.meta
        d_out = d_out.contiguous()
        d_feats = torch.empty((n, cf), dtype=torch.float32, device=d_out.device)
        off = _lib.FgGroupOffsets()
        for k, o in enumerate(offsets):
            off.off[k] = int(o)
        _lib.check(_lib.load().sst_fg_virtual_rows_bwd_f32(_lib.ptr(d_out), d_out.size(0), d_out.size(1), _lib.ptr(slot),
                                                           ctypes.byref(off), n, slot.size(0), cf, _lib.ptr(d_feats),
                                                           _lib.stream_ptr()), 'sst_fg_virtual_rows_bwd_f32')
        return d_feats, None, None, None, None, None, None, None, None


def virtual_rows(sampled, seg_feats, seg_logits, seg_points, pc_range):
    """The projector input of SingleStageFSDV2.extract_feat (:172-176) for the rows ``sampled`` names (the result of
    ``group_sample`` or ``fg_sample``): -> (virtual_input [S, F + 3 + K + (P - 3)] = cat(seg_feats, (clip(centre) - xyz) / 10,
    seg_logits, points[:, 3:]) of every sampled row, clipped centres [S, 3]).  seg_logits and the centres carry no gradient, as the
    reference detaches them (:463-467); seg_feats receives it."""
    for t in (seg_feats, seg_logits, seg_points):
        check_f32_strided(WHERE, t)
    if seg_points.dim() != 2 or seg_points.size(1) < 3:
        raise RuntimeError(f'{WHERE}: seg_points must be [N, >= 3], got {tuple(seg_points.shape)}')
    n = seg_points.size(0)
    if seg_feats.size(0) != n or seg_logits.size(0) != n or tuple(sampled['slot'].shape[1:]) != (n,):
        raise RuntimeError(f'{WHERE}: seg_feats, seg_logits and the sampled slots must have {n} rows')
    off = sampled['class_offsets']
    src = sampled['src_cat']
    centers = sampled['center_cat']                     # the per-group lists are cuts of this one buffer
    lo, hi = clip_bounds(pc_range)
    return _VirtualRows.apply(seg_feats, seg_logits.detach(), seg_points.detach(), centers.detach(), src,
                              sampled['slot'], off, lo, hi)
