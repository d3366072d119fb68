"""The FSD++ incremental point stage: what TwoStageFSDPP puts in front of its segmentor (detectors/two_stage_fsdpp.py:460-755 and
detectors/incremental_ops.py of the reference).  For every sample and every previous frame the points inside the enlarged seed
boxes are cropped and capped per box; then come the points of the current frame, and of frame -1, that fall into voxels no base
frame occupies.  The work runs in csrc/incremental.hip behind the C ABI of include/sst_amd.h; there is no CPU path.

A training batch costs one packed host-to-device copy (the boxes of all (sample, frame) pairs and their offsets), one memset, at
most one sort, a handful of launches and ONE host read (the row counts of every segment, through a pinned buffer).

Order of the rows of a sample (the reference's): crops of frame -1, -2, ... with the appended column float(-i - 1) / 10, then
the delta points with 0, then the delta points of frame -1 with -0.1.  Inside a segment the rows are in ascending input index
(the reference's order there is its random permutation; a voxelisation follows).
"""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from ._head_common import cfg_get as _get

MAX_SAMPLES, MAX_FRAMES, MAX_QUERIES, MAX_CLOUDS, MAX_COLS = 16, 16, 4, 8, 15

REFUSED_CFG = ('n_fps', 'voxel_pooling_size', 'crop_painting', 'virtual_seed_points_cfg', 'noise_cfg', 'pre_nms_thr',
               'elegant_max_age')


def refuse_cfg(incremental_cfg, who='sst_amd.incremental'):
    """the settings of incremental_cfg no shipped config uses: refused by name"""
    for key in REFUSED_CFG:
        val = _get(incremental_cfg, key, None)
        if val is None or val is False or (key == 'pre_nms_thr' and not val > 0):
            continue
        why = ' (the reference calls filter_seed_by_nms, a method it does not define)' if key == 'pre_nms_thr' else ''
        raise NotImplementedError(f'{who}: incremental_cfg.{key} is not built{why}')


def spatial_size(voxel_size, point_cloud_range, fp32=True):
    """incremental_ops.py:58-61 (fp32 tensors) / :105-108 (Python floats): int((hi - lo) / vs) + 1 per axis"""
    if fp32:
        r, v = np.asarray(point_cloud_range, np.float32), np.asarray(voxel_size, np.float32)
        return tuple(int((r[3 + c] - r[c]) / v[c]) + 1 for c in range(3))
    return tuple(int((point_cloud_range[3 + c] - point_cloud_range[c]) / voxel_size[c]) + 1 for c in range(3))


def _f3(vals):
    return (ctypes.c_float * 3)(*[float(v) for v in vals])


def _rows(t, what):
    """a float32 [n, >= 3] device tensor whose rows are contiguous"""
    if not t.is_cuda:
        raise RuntimeError('sst_amd: tensor must be a CUDA/HIP tensor (no CPU path in this library)')
    if t.dtype != torch.float32 or t.dim() != 2 or t.size(1) < 3:
        raise RuntimeError(f'{what}: float32 [n, >= 3] points expected, got {t.dtype} {tuple(t.shape)}')
    return t if (t.stride(1) == 1 or t.size(0) == 0) else t.contiguous()


def voxel_coors(points, voxel_size, point_cloud_range):
    """voxelize_single (incremental_ops.py:14-18): torch.div(p[:, :3] - lo, vs, rounding_mode='floor').int() -> int32 [n, 3]"""
    points = _rows(points, 'voxel_coors')
    n = points.size(0)
    out = torch.empty((n, 3), dtype=torch.int32, device=points.device)
    rc = _lib.load().sst_incr_voxel_coors_f32(_lib.ptr(points), n, points.stride(0) if n else 3, _f3(point_cloud_range[:3]),
                                              _f3(voxel_size), _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, 'sst_incr_voxel_coors_f32')
    return out


def incremental_points_mask(coors1, coors2, spatial_size):
    """torchex.incremental_points_mask: bool [len(coors2)], True where no row of coors1 equals the row of coors2 (the set
    semantics of find_delta_unq_coors + find_delta_pc_mask), exact for every int32 triple, inside the grid or not"""
    _lib.require_cuda(coors1, coors2)
    if coors1.dim() != 2 or coors2.dim() != 2 or coors1.size(1) != 3 or coors2.size(1) != 3:
        raise RuntimeError('incremental_points_mask: [n, 3] coordinates expected')
    coors1, coors2 = coors1.to(torch.int32), coors2.to(torch.int32)
    n1, n2 = coors1.size(0), coors2.size(0)
    mask = torch.empty(n2, dtype=torch.uint8, device=coors2.device)
    sp = _lib.i32array(spatial_size)
    lib = _lib.load()
    nbytes = lib.sst_incr_mask_workspace_bytes(n1, sp)
    _lib.check(min(nbytes, 0), 'sst_incr_mask_workspace_bytes')
    ws = _lib.workspace(nbytes, coors2.device)
    rc = lib.sst_incr_mask_i32(_lib.ptr(coors1), n1, _lib.ptr(coors2), n2, sp, _lib.ptr(ws), ws.numel(), _lib.ptr(mask),
                               _lib.stream_ptr())
    _lib.check(rc, 'sst_incr_mask_i32')
    return mask.bool()


def delta_mask(base_list, query, voxel_size, point_cloud_range, lower_bound=False, grid=None):
    """bool [len(query)]: True where the query point falls into a voxel none of the base clouds' points falls into.  The base
    clouds (up to 8) travel by value: no concatenation.  lower_bound: the filter of find_delta_points_by_voxelization_list_v3."""
    query = _rows(query, 'delta_mask')
    base_list = [_rows(b, 'delta_mask') for b in base_list if b.size(0) > 0]
    if len(base_list) > MAX_CLOUDS:
        base_list = base_list[:MAX_CLOUDS - 1] + [torch.cat([b[:, :3] for b in base_list[MAX_CLOUDS - 1:]], 0)]
    grid = spatial_size(voxel_size, point_cloud_range, fp32=not lower_bound) if grid is None else grid
    a = _lib.IncrDeltaArgs()
    for i, b in enumerate(base_list):
        a.base[i], a.n_base[i], a.ld_base[i] = b.data_ptr(), b.size(0), b.stride(0)
    n_base = sum(b.size(0) for b in base_list)
    mask = torch.empty(query.size(0), dtype=torch.uint8, device=query.device)
    a.query, a.n_query, a.ld_query, a.mask = query.data_ptr(), query.size(0), max(query.stride(0), 3), mask.data_ptr()
    a.n_clouds, a.lower_bound = len(base_list), 1 if lower_bound else 0
    a.lo, a.vs, a.grid = _f3(point_cloud_range[:3]), _f3(voxel_size), _lib.i32array(grid)
    lib = _lib.load()
    nbytes = lib.sst_incr_mask_workspace_bytes(n_base, a.grid)
    _lib.check(min(nbytes, 0), 'sst_incr_mask_workspace_bytes')
    ws = _lib.workspace(nbytes, query.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    _lib.check(lib.sst_incr_delta_mask_f32(ctypes.byref(a), _lib.stream_ptr()), 'sst_incr_delta_mask_f32')
    return mask.bool()


def find_delta_points_by_voxelization(pc1, pc2, voxel_size, pc_range):
    """incremental_ops.py:45-63: the points of pc2 in voxels no point of pc1 occupies"""
    return pc2[delta_mask([pc1], pc2, voxel_size, pc_range)]


def find_delta_points_by_voxelization_list_v3(pc1_list, pc2, voxel_size, pc_range):
    """incremental_ops.py:99-123: the same against a list of clouds; both sides filtered strictly above the lower bounds"""
    return pc2[delta_mask(list(pc1_list), pc2, voxel_size, pc_range, lower_bound=True)]


# ---- frame transforms --------------------------------------------------------------------------------------------------------

def _host64(m):
    if torch.is_tensor(m):
        m = m.detach().cpu().numpy()
    return np.asarray(m, np.float64).reshape(4, 4)


def frame_matrix(pre_pose, cur_pose=None, cur_pose_inv=None):
    """inv(cur_pose) @ pre_pose formed on the host in float64 and rounded to float32 once -> numpy [4, 4] float32"""
    inv = np.linalg.inv(_host64(cur_pose)) if cur_pose_inv is None else _host64(cur_pose_inv)
    return (inv @ _host64(pre_pose)).astype(np.float32)


def transform_clouds(clouds, matrices):
    """every cloud [n, C] moved by its own 4 x 4 (or 3 x 4) matrix, the other columns copied: one launch per 8 clouds, one
    output buffer; -> list of [n, C] views"""
    if len(clouds) != len(matrices):
        raise RuntimeError('transform_clouds: one matrix per cloud expected')
    if not clouds:
        return []
    clouds = [_rows(c, 'transform_clouds') for c in clouds]
    cols = clouds[0].size(1)
    if any(c.size(1) != cols for c in clouds):
        raise RuntimeError('transform_clouds: clouds of one width expected')
    clouds = [c.contiguous() for c in clouds]
    total = sum(c.size(0) for c in clouds)
    buf = torch.empty((total, cols), dtype=torch.float32, device=clouds[0].device)
    outs, o = [], 0
    for c in clouds:
        outs.append(buf[o:o + c.size(0)])
        o += c.size(0)
    lib = _lib.load()
    for g0 in range(0, len(clouds), MAX_CLOUDS):
        a = _lib.FrameTransformArgs()
        group = range(g0, min(g0 + MAX_CLOUDS, len(clouds)))
        for k, i in enumerate(group):
            a.src[k], a.dst[k], a.n[k] = clouds[i].data_ptr(), outs[i].data_ptr(), clouds[i].size(0)
            m = np.asarray(matrices[i], np.float32).reshape(-1, 4)[:3]
            for e, v in enumerate(m.reshape(-1)):
                a.mat[k][e] = float(v)
        a.n_clouds, a.cols = len(group), cols
        _lib.check(lib.sst_points_frame_transform_f32(ctypes.byref(a), _lib.stream_ptr()), 'sst_points_frame_transform_f32')
    return outs


def points_frame_transform(pre_points, pre_pose, cur_pose, cur_pose_inv=None):
    """incremental_ops.py:175-186: [n, 3] points of the frame with pose pre_pose in the frame with pose cur_pose.  The matrix is
    formed on the host in float64 (no device inverse); the last bits differ from the reference's fp32 inverse and matmul."""
    pre_points = _rows(pre_points, 'points_frame_transform')
    return transform_clouds([pre_points[:, :3]], [frame_matrix(pre_pose, cur_pose, cur_pose_inv)])[0]


def _box_tensor(boxes):
    return boxes.tensor if hasattr(boxes, 'tensor') else boxes


def heading_unit_vector(boxes):
    yaw = boxes[:, 6]
    return torch.stack([torch.sin(yaw), torch.cos(yaw), torch.zeros_like(yaw)], 1)


def box_frame_transform_gpu(pre_boxes, pre_pose, cur_pose, cur_pose_inv=None):
    """incremental_ops.py:125-162 on an [n, 7 | 9] tensor (or anything with ``.tensor``; the same kind comes back): centres by
    the full matrix, headings by its rotation, velocities by its rotation.  A few hundred boxes: torch."""
    src = _box_tensor(pre_boxes)
    assert src.size(1) in (7, 9)
    if len(src) == 0:
        return pre_boxes
    mm = torch.as_tensor(frame_matrix(pre_pose, cur_pose, cur_pose_inv)).to(src.device)
    centers = (F.pad(src[:, :3], (0, 1), 'constant', 1) @ mm.T)[:, :3]
    mm_zero_t = mm.clone()
    mm_zero_t[:3, 3] = 0
    heading = (F.pad(heading_unit_vector(src), (0, 1), 'constant', 1) @ mm_zero_t.T)[:, :3]
    yaw = torch.atan2(heading[:, 0], heading[:, 1])
    out = torch.cat([centers, src[:, 3:6], yaw[:, None]], 1)
    if src.size(1) == 9:
        velo = F.pad(src[:, [7, 8]], (0, 1), 'constant', 0) @ mm[:3, :3].T
        out = torch.cat([out, velo[:, :2]], 1)
    if hasattr(pre_boxes, 'tensor'):
        return pre_boxes.new_box(out) if hasattr(pre_boxes, 'new_box') else type(pre_boxes)(out, box_dim=out.size(1))
    return out


# ---- seed boxes --------------------------------------------------------------------------------------------------------------

def _host_np(x, dtype):
    x = _box_tensor(x)
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype)


def pack_seed_info(seed_info, incremental_cfg, n_frames):
    """the seed boxes of all (sample, frame) pairs as one host array -> (rows float32 [B, 8] = box | extra width of the box,
    offsets int32 [S * n_frames + 1]): the boxes of (sample s, frame -(i + 1)) are rows offsets[s * n_frames + i] ..  A sample
    with fewer frames, or a frame without boxes, has empty segments.  extra_width may be a dictionary by label."""
    extra = _get(incremental_cfg, 'extra_width', 0.0)
    rows, offsets = [], [0]
    for frames in seed_info:
        for i in range(n_frames):
            n = 0
            if i < len(frames):
                b = _host_np(frames[i]['gt_bboxes_3d'], np.float32).reshape(-1, _box_cols(frames[i]['gt_bboxes_3d']))[:, :7]
                n = b.shape[0]
                if n:
                    if isinstance(extra, dict):
                        labels = _host_np(frames[i]['gt_labels_3d'], np.float32).reshape(-1)
                        if labels.shape[0] != n:
                            raise RuntimeError('pack_seed_info: one label per seed box expected')
                        ew = np.asarray([extra[l] for l in labels.tolist()], np.float32)
                    else:
                        ew = np.full((n,), float(extra), np.float32)
                    rows.append(np.concatenate([b, ew[:, None]], 1))
            offsets.append(offsets[-1] + n)
    rows = np.concatenate(rows, 0) if rows else np.zeros((0, 8), np.float32)
    return rows, np.asarray(offsets, np.int32)


def _box_cols(boxes):
    t = _box_tensor(boxes)
    return int(t.shape[-1]) if getattr(t, 'ndim', 1) > 1 and t.shape[-1] > 0 else 7


def _upload(rows, offsets, dev):
    """one pinned host buffer, one copy -> (boxes [B, 8] float32, offsets int32) views of one device buffer"""
    nb, no = rows.size * 4, offsets.size * 4
    host = torch.empty(max(nb + no, 4), dtype=torch.uint8)
    if torch.cuda.is_available():
        host = host.pin_memory()
    host[:nb].view(torch.float32)[:] = torch.from_numpy(np.ascontiguousarray(rows).reshape(-1))
    host[nb:nb + no].view(torch.int32)[:] = torch.from_numpy(np.ascontiguousarray(offsets))
    buf = host.to(dev, non_blocking=True)
    return buf[:nb].view(torch.float32).view(-1, 8), buf[nb:nb + no].view(torch.int32)


def modify_boxes(boxes8, incremental_cfg, training):
    """modify_previous_boxes (:763-798) once on the boxes of the whole batch: the training noise (skipped when all three
    settings are 0: the reference's arithmetic is the identity there), then the enlargement -> [B, 7]"""
    b, ew = boxes8[:, :7].clone(), boxes8[:, 7]
    if training:
        cn, dn, yn = (_get(incremental_cfg, k, 0.0) for k in ('center_noise', 'dim_noise', 'yaw_noise'))
        if any(isinstance(v, (list, tuple)) for v in (cn, dn)):
            raise NotImplementedError('sst_amd.incremental: per-axis center_noise / dim_noise (the reference reads an undefined '
                                      'name there)')
        if cn != 0 or dn != 0 or yn != 0:
            num, dev = b.size(0), b.device
            dims = b[:, 3:6].clone()
            cen = (torch.rand((num, 3), dtype=b.dtype, device=dev) - 0.5) * 2 * cn * dims
            dim = (torch.rand((num, 3), dtype=b.dtype, device=dev) - 0.5) * 2 * dn + 1
            yaw = (torch.rand((num,), dtype=b.dtype, device=dev) - 0.5) * 2 * yn
            b[:, :3] += cen
            b[:, 3:6] *= dim
            b[:, 6] += yaw
    b[:, 3:6] += ew[:, None] * 2
    b[:, 2] -= ew
    return b


def enlarge_boxes(boxes, labels, incremental_cfg, training):
    """modify_previous_boxes for one device box tensor [n, 7 | 9] -> [n, 7] (the sequential path)"""
    boxes = _box_tensor(boxes)[:, :7].float()
    extra = _get(incremental_cfg, 'extra_width', 0.0)
    if isinstance(extra, dict):
        lab = labels.detach().cpu().tolist() if torch.is_tensor(labels) else np.asarray(labels).tolist()
        ew = torch.tensor([float(extra[l]) for l in lab], dtype=torch.float32).to(boxes.device)
    else:
        ew = torch.full((boxes.size(0),), float(extra), dtype=torch.float32, device=boxes.device)
    return modify_boxes(torch.cat([boxes, ew[:, None]], 1), incremental_cfg, training)


# ---- the stage ---------------------------------------------------------------------------------------------------------------

class _Workspace(object):
    """the stage's one reusable device workspace and its pinned count words, per device"""
    cache = {}

    @classmethod
    def get(cls, dev, nbytes, n_counts):
        ent = cls.cache.get(dev)
        if ent is None or ent[0].numel() < nbytes or ent[1].numel() < n_counts:
            ws = torch.empty(max(int(nbytes * 1.25), 256), dtype=torch.uint8, device=dev)
            pin = torch.empty(max(n_counts, 64), dtype=torch.int32)
            if torch.cuda.is_available():
                pin = pin.pin_memory()
            ent = cls.cache[dev] = (ws, pin)
        return ent


def stage(points, pts_frame_inds, boxes, box_offsets, n_frames, queries, voxel_size, point_cloud_range, max_crop_points=0,
          keys=None, lower_bound=False, fallback=None):
    """the kernels of the stage for a batch.  points / pts_frame_inds: per sample [n, C] float32 and [n] integer device tensors;
    boxes [B, 7] (enlarged) with box_offsets int32 [S * n_frames + 1] on the device; queries: list of (inc_frame, base_lo,
    base_hi, tag); keys: one integer tensor for the whole batch (its low 32 bits are the key) or None (key = point index).
    fallback(s) -> [k, C + 1] rows that replace the crops of a sample without any (or None).
    -> (out [M, C + 1], per-sample views, counts numpy int32 [S, n_frames + len(queries)])"""
    S = len(points)
    if S == 0:
        return None, [], np.zeros((0, n_frames + len(queries)), np.int32)
    if S > MAX_SAMPLES or n_frames > MAX_FRAMES or len(queries) > MAX_QUERIES:
        raise RuntimeError(f'sst_amd.incremental.stage: at most {MAX_SAMPLES} samples, {MAX_FRAMES} crop frames and {MAX_QUERIES} '
                           'queries')
    points = [_rows(p, 'incremental.stage').contiguous() for p in points]
    dev, C = points[0].device, points[0].size(1)
    if any(p.size(1) != C for p in points) or C > MAX_COLS:
        raise RuntimeError(f'sst_amd.incremental.stage: points of one width <= {MAX_COLS} expected')
    finds = []
    for p, f in zip(points, pts_frame_inds):
        _lib.require_cuda(f)
        if f.numel() != p.size(0):
            raise RuntimeError('sst_amd.incremental.stage: one frame index per point expected')
        finds.append(f if f.dtype == torch.long else f.long())
    nb = n_frames + len(queries)
    total = sum(p.size(0) for p in points)
    a = _lib.IncrArgs()
    for s in range(S):
        a.points[s], a.frame_inds[s], a.n_points[s] = points[s].data_ptr(), finds[s].data_ptr(), points[s].size(0)
    n_boxes = int(boxes.size(0)) if boxes is not None else 0
    if n_boxes and n_frames:
        boxes = boxes.contiguous()
        a.boxes, a.box_offsets = boxes.data_ptr(), box_offsets.data_ptr()
    if keys is not None:
        _lib.require_cuda(keys)
        if keys.numel() != total:
            raise RuntimeError('sst_amd.incremental.stage: one key per point of the batch expected')
        keys = keys.to(torch.int64).to(torch.int32) if keys.dtype not in (torch.int32,) else keys
        a.keys = keys.data_ptr()
    a.n_samples, a.cols, a.n_frames, a.n_queries, a.n_boxes = S, C, n_frames, len(queries), n_boxes
    a.max_crop_points, a.lower_bound = int(max_crop_points or 0), 1 if lower_bound else 0
    for q, (inc, lo, hi, tag) in enumerate(queries):
        a.q_inc[q], a.q_lo[q], a.q_hi[q], a.q_tag[q] = int(inc), int(lo), int(hi), float(tag)
    a.lo, a.vs = _f3(point_cloud_range[:3]), _f3(voxel_size)
    a.grid = _lib.i32array(spatial_size(voxel_size, point_cloud_range, fp32=not lower_bound))
    lib = _lib.load()
    nbytes = lib.sst_incr_workspace_bytes(ctypes.byref(a))
    _lib.check(min(nbytes, 0), 'sst_incr_workspace_bytes')
    ws, pin = _Workspace.get(dev, nbytes, S * nb)
    counts_d = torch.empty((S, nb), dtype=torch.int32, device=dev)
    a.workspace, a.workspace_bytes, a.counts = ws.data_ptr(), ws.numel(), counts_d.data_ptr()
    _lib.check(lib.sst_incr_plan_f32(ctypes.byref(a), _lib.stream_ptr()), 'sst_incr_plan_f32')
    # the one host read of the stage
    host = pin[:S * nb].view(S, nb)
    host.copy_(counts_d, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    counts = host.numpy().copy()
    extra = [None] * S
    if fallback is not None and n_frames > 0:
        for s in range(S):
            if counts[s, :n_frames].sum() == 0:
                extra[s] = fallback(s)
    bases, sample_rows, m = [], [], 0
    for s in range(S):
        start = m
        if extra[s] is not None:
            m += extra[s].size(0)
        for b in range(nb):
            bases.append(m)
            m += int(counts[s, b])
        sample_rows.append((start, m))
    out = torch.empty((m, C + 1), dtype=torch.float32, device=dev)
    for i, v in enumerate(bases):
        a.seg_base[i] = v
    a.out = out.data_ptr()
    if m:
        _lib.check(lib.sst_incr_rows_f32(ctypes.byref(a), _lib.stream_ptr()), 'sst_incr_rows_f32')
    for s in range(S):
        if extra[s] is not None and extra[s].size(0):
            out[sample_rows[s][0]:sample_rows[s][0] + extra[s].size(0)] = extra[s]
    return out, [out[lo:hi] for lo, hi in sample_rows], counts


def seed_crop(points, boxes, max_crop_points=0, keys=None):
    """crop_and_process_points (:637-678) of one cloud against one set of (already enlarged) boxes [n, 7]: the points inside a
    box, capped per box at the max_crop_points smallest (key, index), in ascending index -> [k, C]"""
    points = _rows(points, 'seed_crop')
    boxes = _box_tensor(boxes)
    if points.size(0) == 0 or len(boxes) == 0:
        return points.new_zeros((0, points.size(1)))
    boxes = boxes[:, :7].float().contiguous()
    _lib.require_cuda(boxes)
    finds = torch.full((points.size(0),), -1, dtype=torch.long, device=points.device)
    offsets = torch.tensor([0, boxes.size(0)], dtype=torch.int32).to(points.device)
    out, _, _ = stage([points], [finds], boxes, offsets, 1, [], (1, 1, 1), (0, 0, 0, 1, 1, 1), max_crop_points, keys)
    return out[:, :-1]


def queries_of(incremental_cfg, max_pre_frames):
    """the delta queries of generate_points (:475-492) as (inc_frame, base_lo, base_hi, tag)"""
    if _get(incremental_cfg, 'disable_incremental', False):
        return []
    num_base = _get(incremental_cfg, 'num_base_frame', max_pre_frames)
    lo = -min(int(num_base), int(max_pre_frames))
    q = [(0, lo, -1, 0.0)]
    if _get(incremental_cfg, 'max_age', 0) > 0:
        q.append((-1, lo, -2, -0.1))
    return q


def generate_points(points, pts_frame_inds, seed_info, incremental_cfg, training, keys=None):
    """TwoStageFSDPP.generate_points (:460-503) for a whole batch -> (out_points_list, num_delta_points_list).

    points / pts_frame_inds: per sample [n, C] and [n] device tensors; seed_info: per sample the list over previous frames
    (frame -1 first) of dict(gt_bboxes_3d, gt_labels_3d, scores) on the host (already cut by preprocess_seed).  keys: the random
    32-bit keys of crop_shuffle, one per point of the batch in sample order (default: drawn here on the device when crop_shuffle
    is set).  The per-sample outputs are views of one buffer."""
    refuse_cfg(incremental_cfg, 'sst_amd.incremental.generate_points')
    for p in points:
        if not p.is_cuda:
            raise RuntimeError('sst_amd: tensor must be a CUDA/HIP tensor (no CPU path in this library)')
    S = len(points)
    if len(seed_info) != S or len(pts_frame_inds) != S:
        raise RuntimeError('generate_points: one frame-index tensor and one seed list per sample expected')
    max_pre = int(_get(incremental_cfg, 'num_previous_frames', 4))
    frames_of = []
    for frames in seed_info:
        assert isinstance(frames, (list, tuple)) and len(frames) >= 1, 'frame-wise list'
        n = min(len(frames), max_pre)
        crop_frames = _get(incremental_cfg, 'crop_frames', None)
        frames_of.append(min(int(crop_frames), n) if crop_frames is not None else n)
    n_frames = max(frames_of) if frames_of else 0
    dev = points[0].device
    rows, offsets = pack_seed_info([f[:k] for f, k in zip(seed_info, frames_of)], incremental_cfg, n_frames)
    boxes8, d_offsets = _upload(rows, offsets, dev)
    boxes = modify_boxes(boxes8, incremental_cfg, training) if rows.shape[0] else boxes8[:, :7]
    max_n = int(_get(incremental_cfg, 'max_crop_points', 0) or 0)
    if keys is None and max_n > 0 and _get(incremental_cfg, 'crop_shuffle', False):
        keys = torch.randint(0, 2 ** 32, (sum(p.size(0) for p in points),), dtype=torch.int64, device=dev)
    if max_n <= 0 or not _get(incremental_cfg, 'crop_shuffle', False):
        keys = None
    queries = queries_of(incremental_cfg, max_pre)

    def fallback(s):
        """:629-632, the rare sample without a single cropped point: rows 1 .. 199 of its previous-frame points"""
        f = pts_frame_inds[s]
        pre = points[s][(f < 0) & (f >= -max_pre)]
        return F.pad(pre[1:200, :], (0, 1), 'constant', float(-frames_of[s]) / 10)

    _, outs, counts = stage(points, pts_frame_inds, boxes, d_offsets, n_frames, queries, _get(incremental_cfg, 'voxel_size'),
                            _get(incremental_cfg, 'point_cloud_range'), max_n, keys, fallback=fallback)
    num_delta = [int(counts[s, n_frames:].sum()) for s in range(S)] if queries else []
    return outs, num_delta
