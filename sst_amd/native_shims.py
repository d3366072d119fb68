"""Drop-in replacements for the NATIVE modules the reference's Python imports - integration path B of INTEGRATION.md:
every reference .py file stays as it is, only the compiled extensions are swapped.

    import sst_amd.native_shims as shims, sys
    sys.modules['mmdet3d.ops.voxel.voxel_layer'] = shims.voxel_layer            # voxelization.cpp:6-11 (pybind module)
    sys.modules['ingroup_indices'] = shims.ingroup_indices                      # TorchEx, call site sst_ops.py:249-257
    sys.modules['dynamic_point_pool_ext'] = shims.dynamic_point_pool_ext        # TorchEx, dynamic_point_pool_op.py:36, 86-88
    sys.modules['mmdet3d.ops.spconv.sparse_conv_ext'] = shims.sparse_conv_ext   # ops/spconv/ops.py:93-183
    sys.modules['torch_scatter'] = shims.torch_scatter                          # sst_ops.py:172-177
    sys.modules['mmdet3d.ops.iou3d.iou3d_cuda'] = shims.iou3d_cuda              # iou3d_utils.py, base_box3d.py:395-450
    sys.modules['mmdet3d.ops.roiaware_pool3d.roiaware_pool3d_ext'] = shims.roiaware_pool3d_ext  # points_in_boxes.py
    sys.modules['torchex'] = shims.torchex                                      # TorchEx, lidar_box3d.py:5-12
    sys.modules['mmdet3d.ops.furthest_point_sample.furthest_point_sample_ext'] = shims.furthest_point_sample_ext
                                                                                # furthest_point_sample.py:4, 32-33, 67-68
    sys.modules['mmcv.ops.deform_conv'] = shims.mmcv_deform_conv                # mmcv's 'DCN': centerpoint_head.py:168-170

Each namespace has exactly the functions, argument orders and in / out conventions of the module it stands for (outputs
the reference pre-allocates are written in place).  Everything runs on the GPU through the C ABI of libsst_amd.so
(`sst_amd/_lib.py`); there is no CPU path, as in the reference (`voxelization.h:106`).  Executed by
tests/test_gpu_native_shims.py.
"""
import types

import torch

from . import _lib
from . import box_ops as _box
from . import deform_conv as _dcn
from . import fps as _fps
from . import incremental as _incr
from . import kernels as K
from . import spconv as _spconv
from . import voxel as _voxel
from .dynamic_point_pool import _pool
from .sst_ops import plan_of_inverse


# ------------------------------------------------------------------------------------------------------------------
# mmdet3d/ops/voxel/voxel_layer  (src/voxelization.h:71-128)
# ------------------------------------------------------------------------------------------------------------------
def _dynamic_point_to_voxel_backward(grad_feats, grad_reduced_feats, feats, reduced_feats, coors_idx, reduce_count,
                                     reduce_type):
    """scatter_points_cuda.cu:236-303: writes grad_feats in place.  coors_idx = the forward's coors_map (-1: the point's
    voxel was discarded), reduce_count = points per kept voxel.  MAX: the gradient of a (voxel, channel) goes to the
    point with the smallest index whose feature equals the maximum (max_reduce_traceback_scatter_idx_kernel)."""
    if reduce_type not in ('max', 'sum', 'mean'):
        raise RuntimeError('do not support reduce type ' + str(reduce_type))
    _lib.require_cuda(grad_feats, grad_reduced_feats, feats, reduced_feats, coors_idx)
    n, c = feats.shape
    grad_feats.zero_()
    if n == 0 or reduced_feats.size(0) == 0:
        return
    valid = coors_idx >= 0
    row = coors_idx.clamp(min=0).long()
    g = grad_reduced_feats[row]
    if reduce_type == 'mean':
        g = g / reduce_count[row].to(g.dtype).unsqueeze(1)
    if reduce_type in ('sum', 'mean'):
        grad_feats.copy_(torch.where(valid.unsqueeze(1), g, torch.zeros_like(g)))
        return
    ar = torch.arange(n, device=feats.device).unsqueeze(1).expand(n, c)
    hit = (feats == reduced_feats[row]) & valid.unsqueeze(1)
    cand = torch.where(hit, ar, torch.full_like(ar, n))
    first = torch.full((reduced_feats.size(0), c), n, dtype=cand.dtype, device=feats.device)
    first.scatter_reduce_(0, row.unsqueeze(1).expand(n, c), cand, 'amin', include_self=True)
    take = (first[row] == ar) & valid.unsqueeze(1)
    grad_feats.copy_(torch.where(take, g, torch.zeros_like(g)))


voxel_layer = types.SimpleNamespace(
    dynamic_voxelize=_voxel.dynamic_voxelize,                               # (points, coors, voxel_size, coors_range, NDim=3)
    hard_voxelize=_voxel.hard_voxelize,
    dynamic_point_to_voxel_forward=_voxel.dynamic_point_to_voxel_forward,   # -> [reduced, out_coors, coors_map, count]
    dynamic_point_to_voxel_backward=_dynamic_point_to_voxel_backward)


# ------------------------------------------------------------------------------------------------------------------
# TorchEx ingroup_indices
# ------------------------------------------------------------------------------------------------------------------
def _ingroup_forward(group_inds, out_inds):
    """out_inds (int64, pre-filled with -1 by the caller) <- rank of every element inside its group"""
    out_inds.copy_(K.ingroup_rank(group_inds.contiguous()))


ingroup_indices = types.SimpleNamespace(forward=_ingroup_forward)


# ------------------------------------------------------------------------------------------------------------------
# TorchEx dynamic_point_pool_ext
# ------------------------------------------------------------------------------------------------------------------
def _dpp_forward(rois, pts, extra_wlh, max_inbox_point, out_pts_idx, out_roi_idx, out_pts_feats, rois_batch=None,
                 pts_batch=None):
    """outputs are the caller's pre-filled tensors (-1, -1, zeros): the pairs found are written as a prefix, the rest
    stays untouched - the reference then masks out_pts_idx >= 0 (dynamic_point_pool_op.py:38-40)"""
    a, b, f, n = _pool(rois, rois_batch, pts, pts_batch, extra_wlh, max_inbox_point, out_pts_idx.numel())
    out_pts_idx.copy_(a)
    out_roi_idx.copy_(b)
    out_pts_feats.copy_(f)
    return n


def _dpp_mixed(rois, rois_batch, pts, pts_batch, extra_wlh, max_inbox_point, out_pts_idx, out_roi_idx, out_pts_feats):
    return _dpp_forward(rois, pts, extra_wlh, max_inbox_point, out_pts_idx, out_roi_idx, out_pts_feats, rois_batch,
                        pts_batch)


dynamic_point_pool_ext = types.SimpleNamespace(forward=_dpp_forward, dynamic_point_pool_mixed_gpu=_dpp_mixed)


# ------------------------------------------------------------------------------------------------------------------
# mmdet3d/ops/spconv/sparse_conv_ext  (3-D, int32 indices, fp32; ops/spconv/ops.py:93-183)
# ------------------------------------------------------------------------------------------------------------------
def _get_indice_pairs_3d(indices, batch_size, out_shape, spatial_shape, ksize, stride, padding, dilation, out_padding,
                         subm, transpose):
    return list(_spconv.get_indice_pairs(indices, batch_size, spatial_shape, ksize, stride, padding, dilation,
                                         out_padding, bool(subm), bool(transpose)))


def _indice_conv_fp32(features, filters, indice_pairs, indice_pair_num, num_activate_out, inverse, subm):
    return _spconv.indice_conv(features, filters, indice_pairs, indice_pair_num, num_activate_out, bool(inverse),
                               bool(subm))


def _indice_conv_backward_fp32(features, filters, out_bp, indice_pairs, indice_pair_num, inverse, subm):
    return list(_spconv.indice_conv_backward(features, filters, out_bp, indice_pairs, indice_pair_num, bool(inverse),
                                             bool(subm)))


sparse_conv_ext = types.SimpleNamespace(
    get_indice_pairs_3d=_get_indice_pairs_3d, indice_conv_fp32=_indice_conv_fp32,
    indice_conv_backward_fp32=_indice_conv_backward_fp32, indice_maxpool_fp32=_spconv.indice_maxpool,
    indice_maxpool_backward_fp32=_spconv.indice_maxpool_backward)


# ------------------------------------------------------------------------------------------------------------------
# torch_scatter: the two functions sst_ops.py:172-177 calls (dim = 0, index = the inverse map of a unique)
# ------------------------------------------------------------------------------------------------------------------
def _groups_of(index, src):
    if index.dim() != 1 or index.numel() != src.size(0):
        raise RuntimeError('torch_scatter shim: a 1-D index over dim 0 is expected (the reference passes unq_inv)')
    m = int(index.max().item()) + 1 if index.numel() else 0
    return plan_of_inverse(index, m), m


def _scatter_max(src, index, dim=0):
    """-> (out [G, C], argmax [G, C] int64): row index of the first point attaining the maximum"""
    assert dim == 0
    flat = src.reshape(src.size(0), -1).contiguous().float()
    plan, m = _groups_of(index, flat)
    out, arg = K.segment_argmax(flat, plan)
    return out.reshape((m,) + src.shape[1:]).to(src.dtype), arg.long().reshape((m,) + src.shape[1:])


def _scatter(src, index, dim=0, reduce='sum'):
    assert dim == 0
    if reduce not in ('sum', 'add', 'mean'):
        raise NotImplementedError(reduce)
    flat = src.reshape(src.size(0), -1).contiguous().float()
    plan, m = _groups_of(index, flat)
    out = K.segment_reduce(flat, plan, 'mean' if reduce == 'mean' else 'sum')
    return out.reshape((m,) + src.shape[1:]).to(src.dtype)


torch_scatter = types.SimpleNamespace(scatter_max=_scatter_max, scatter=_scatter)


# ------------------------------------------------------------------------------------------------------------------
# mmdet3d/ops/iou3d/iou3d_cuda  (src/iou3d.cpp:34-185)
# ------------------------------------------------------------------------------------------------------------------
def _fill_pairwise(mode, boxes_a, boxes_b, ans):
    """ans: the caller's [M, N] fp32 device tensor, written in place (CHECK_INPUT on all three, iou3d.cpp:34-78)"""
    _box._check_boxes(boxes_a, 5, 'iou3d_cuda')
    _box._check_boxes(boxes_b, 5, 'iou3d_cuda')
    _box._check_f32(ans)
    if not ans.is_contiguous():
        raise RuntimeError('iou3d_cuda: the output must be contiguous')
    if tuple(ans.shape) != (boxes_a.size(0), boxes_b.size(0)):
        raise RuntimeError(f'iou3d_cuda: output of shape {tuple(ans.shape)} for {boxes_a.size(0)} x {boxes_b.size(0)} boxes')
    if ans.numel():
        _lib.check(_lib.load().sst_boxes_overlap_bev_f32(_lib.ptr(boxes_a), boxes_a.size(0), _lib.ptr(boxes_b),
                                                         boxes_b.size(0), mode, _lib.ptr(ans), _lib.stream_ptr()),
                   'iou3d_cuda')
    return 1


def _nms_into(rotated, boxes, keep, nms_overlap_thresh, device_id=None):
    """keep: the caller's CPU int64 [N] (iou3d.cpp:95-147): the first num_out entries are written; returns num_out"""
    _box._check_boxes(boxes, 5, 'iou3d_cuda.nms')
    if keep.is_cuda or keep.dtype != torch.int64 or not keep.is_contiguous() or keep.numel() < boxes.size(0):
        raise RuntimeError('iou3d_cuda.nms: keep must be a contiguous CPU int64 tensor of at least N entries')
    kept, num = _box.nms_sorted(boxes, nms_overlap_thresh, rotated=rotated)
    if num:
        keep[:num].copy_(kept)
    return num


iou3d_cuda = types.SimpleNamespace(
    boxes_overlap_bev_gpu=lambda a, b, ans: _fill_pairwise(_box.BOX_OVERLAP, a, b, ans),
    boxes_iou_bev_gpu=lambda a, b, ans: _fill_pairwise(_box.BOX_IOU, a, b, ans),
    nms_gpu=lambda boxes, keep, thresh, device_id=None: _nms_into(True, boxes, keep, thresh, device_id),
    nms_normal_gpu=lambda boxes, keep, thresh, device_id=None: _nms_into(False, boxes, keep, thresh, device_id))


# ------------------------------------------------------------------------------------------------------------------
# mmdet3d/ops/roiaware_pool3d/roiaware_pool3d_ext  (src/points_in_boxes_cuda.cu:24-105); boxes come first
# ------------------------------------------------------------------------------------------------------------------
def _not_ported(name):
    def _raise(*args, **kwargs):
        raise RuntimeError(f'roiaware_pool3d_ext.{name} is not provided by sst_amd: it has no caller on the SST / FSD '
                           'path (RoIAwarePool3d is used by PartA2 only; points_in_boxes_cpu by data tools)')
    return _raise


roiaware_pool3d_ext = types.SimpleNamespace(
    points_in_boxes_gpu=lambda boxes, pts, out: _box._points_in_boxes_into(boxes, pts, out, _box.PIB_FIRST),
    points_in_boxes_batch=lambda boxes, pts, out: _box._points_in_boxes_into(boxes, pts, out, _box.PIB_MEMBERSHIP),
    points_in_boxes_cpu=_not_ported('points_in_boxes_cpu'), forward=_not_ported('forward'),
    backward=_not_ported('backward'))


# ------------------------------------------------------------------------------------------------------------------
# mmdet3d/ops/furthest_point_sample/furthest_point_sample_ext  (src/furthest_point_sample.cpp: both wrappers take
# (B, N, m, input, temp, idx) and write idx, the caller's int32 [B, m])
# ------------------------------------------------------------------------------------------------------------------
def _fps_wrapper(b, n, m, points_tensor, temp_tensor, idx_tensor):
    if points_tensor.dim() != 3 or tuple(points_tensor.shape[:2]) != (b, n):
        raise RuntimeError(f'furthest_point_sampling_wrapper: points of shape {tuple(points_tensor.shape)} for B = {b}, N = {n}')
    _fps._fps_into(points_tensor, m, temp_tensor, idx_tensor, 'furthest_point_sampling_wrapper')
    return 1


def _fps_with_dist_wrapper(b, n, m, points_tensor, temp_tensor, idx_tensor):
    if points_tensor.dim() != 3 or tuple(points_tensor.shape) != (b, n, n):
        raise RuntimeError(f'furthest_point_sampling_with_dist_wrapper: distances of shape {tuple(points_tensor.shape)} for '
                           f'B = {b}, N = {n}')
    _fps._fps_with_dist_into(points_tensor, m, temp_tensor, idx_tensor, 'furthest_point_sampling_with_dist_wrapper')
    return 1


furthest_point_sample_ext = types.SimpleNamespace(furthest_point_sampling_wrapper=_fps_wrapper,
                                                  furthest_point_sampling_with_dist_wrapper=_fps_with_dist_wrapper)


# ------------------------------------------------------------------------------------------------------------------
# mmcv.ops.deform_conv: the function and the two modules ('DCN' of mmcv's CONV_LAYERS is DeformConv2dPack).  mmcv's
# deform_conv2d takes (input, offset, weight, stride, padding, dilation, groups, deform_groups, bias=False, im2col_step=32):
# im2col_step only sizes mmcv's column buffer, which this operator does not have
# ------------------------------------------------------------------------------------------------------------------
def _deform_conv2d(input, offset, weight, stride=1, padding=0, dilation=1, groups=1, deform_groups=1, bias=False, im2col_step=32):
    if bias:
        raise NotImplementedError('deform_conv2d: bias=True is not built')
    return _dcn.deform_conv2d(input, offset, weight, stride, padding, dilation, groups, deform_groups)


mmcv_deform_conv = types.SimpleNamespace(deform_conv2d=_deform_conv2d, DeformConv2d=_dcn.DeformConv2d,
                                         DeformConv2dPack=_dcn.DeformConv2dPack)


# ------------------------------------------------------------------------------------------------------------------
# TorchEx: boxes_overlap_1to1 and incremental_points_mask (incremental_ops.py:9-12).  `from torchex import connected_components`
# must keep raising ImportError: the reference falls back to scipy on it (single_stage_fsd.py:19-22).
# ------------------------------------------------------------------------------------------------------------------
torchex = types.ModuleType('torchex', 'sst_amd stand-in for TorchEx: boxes_overlap_1to1 and incremental_points_mask')
torchex.boxes_overlap_1to1 = _box.boxes_overlap_1to1
torchex.incremental_points_mask = _incr.incremental_points_mask
