"""The FSD++ incremental point stage restated with torch ops on the device, the way the reference runs it
(detectors/two_stage_fsdpp.py:460-755, detectors/incremental_ops.py): a Python loop over samples and frames, points_in_boxes,
boolean compactions, the permutation argsort(keys) in place of randperm, the stable in-group rank in place of get_inner_win_inds,
torch.div(..., rounding_mode='floor') for the voxel coordinates and the set formulation (find_delta_unq_coors +
find_delta_pc_mask) for the TorchEx op incremental_points_mask.  It is the bit-for-bit yardstick of tests/test_gpu_incremental.py
and the counterpart tools/incremental_bench.py times.  Inside a segment the rows are sorted by input index (the reference's order
there is its random permutation)."""
import numpy as np
import torch
import torch.nn.functional as F


def voxelize_single(points, voxel_size, pc_range):
    """incremental_ops.py:14-18"""
    return torch.div(points[:, :3] - pc_range[None, :3], voxel_size[None, :], rounding_mode='floor').int()


def spatial_size(voxel_size, pc_range):
    return tuple(int((pc_range[3 + c] - pc_range[c]) / voxel_size[c]) + 1 for c in range(3))


def incremental_points_mask(coors1, coors2, spatial_size=None):
    """the in-tree set semantics of the TorchEx op: a row of coors2 is new iff no row of coors1 equals it"""
    n1 = coors1.size(0)
    if coors2.size(0) == 0:
        return torch.zeros(0, dtype=torch.bool, device=coors2.device)
    _, inv = torch.unique(torch.cat([coors1, coors2], 0), return_inverse=True, dim=0)
    present = torch.zeros(int(inv.max()) + 1, dtype=torch.bool, device=coors2.device)
    present[inv[:n1]] = True
    return ~present[inv[n1:]]


def _dev(vals, device):
    return torch.tensor([float(v) for v in vals], dtype=torch.float32, device=device)


def find_delta_points_by_voxelization(pc1, pc2, voxel_size, pc_range, return_mask=False):
    """incremental_ops.py:45-63"""
    vs, rng = _dev(voxel_size, pc1.device), _dev(pc_range, pc1.device)
    mask = incremental_points_mask(voxelize_single(pc1, vs, rng), voxelize_single(pc2, vs, rng))
    return mask if return_mask else pc2[mask]


def find_delta_points_by_voxelization_list_v3(pc1_list, pc2, voxel_size, pc_range, return_mask=False):
    """incremental_ops.py:99-123; the mask is over the rows of pc2 (False where the lower-bound filter drops the point)"""
    vs, rng = _dev(voxel_size, pc2.device), _dev(pc_range, pc2.device)
    pc1 = torch.cat(pc1_list, 0)
    m1 = (pc1[:, 0] > rng[0]) & (pc1[:, 1] > rng[1]) & (pc1[:, 2] > rng[2])
    m2 = (pc2[:, 0] > rng[0]) & (pc2[:, 1] > rng[1]) & (pc2[:, 2] > rng[2])
    sub = incremental_points_mask(voxelize_single(pc1[m1], vs, rng), voxelize_single(pc2[m2], vs, rng))
    if not return_mask:
        return pc2[m2][sub]
    full = torch.zeros(pc2.size(0), dtype=torch.bool, device=pc2.device)
    full[m2.nonzero().reshape(-1)[sub]] = True
    return full


def stable_ingroup_rank(group):
    """rank[i] = number of j < i with group[j] == group[i] (get_inner_win_inds, the stable choice)"""
    n = group.numel()
    if n == 0:
        return group.new_zeros(0, dtype=torch.long)
    gs, order = torch.sort(group, stable=True)
    pos = torch.arange(n, device=group.device)
    first = torch.ones(n, dtype=torch.bool, device=group.device)
    first[1:] = gs[1:] != gs[:-1]
    start = torch.cummax(torch.where(first, pos, torch.zeros_like(pos)), 0)[0]
    rank = torch.empty(n, dtype=torch.long, device=group.device)
    rank[order] = pos - start
    return rank


def key32(keys):
    """the low 32 bits of integer keys as non-negative int64"""
    return keys.long() & 0xffffffff


def crop_indices(points, boxes, max_n=0, keys=None):
    """crop_and_process_points (:637-678) -> the kept input indices in ascending order.  boxes: enlarged [n, 7]; keys: one per
    point (the permutation is argsort(keys), ties by index) or None (no shuffle)."""
    import sst_amd
    if points.size(0) == 0 or boxes.size(0) == 0:
        return torch.zeros(0, dtype=torch.long, device=points.device)
    box_inds = sst_amd.points_in_boxes_gpu(points[None, :, :3].contiguous(), boxes[None, :, :7].contiguous())[0].long()
    idx = (box_inds > -1).nonzero().reshape(-1)
    pos_box = box_inds[idx]
    if idx.numel() == 0:
        return idx
    if max_n > 0:
        if keys is not None:
            order = torch.sort(key32(keys)[idx], stable=True)[1]
            pos_box, idx = pos_box[order], idx[order]
        valid = stable_ingroup_rank(pos_box) < max_n
        idx = idx[valid]
    return torch.sort(idx)[0]


def enlarged(boxes, extra_width, labels=None):
    """LiDARInstance3DBoxes.enlarged_box / classwise_enlarged_box (lidar_box3d.py:269-307) on a device tensor"""
    out = boxes[:, :7].clone()
    if isinstance(extra_width, dict):
        ew = out.new_ones(len(out))
        for l in torch.unique(labels).tolist():
            ew[labels == l] = extra_width[l]
        out[:, 3:6] += ew[:, None] * 2
        out[:, 2] -= ew
    else:
        out[:, 3:6] += extra_width * 2
        out[:, 2] -= extra_width
    return out


def generate_points(points, pts_frame_inds, seed_info, cfg, keys=None, counters=None):
    """generate_points (:460-503) + get_old_points (:592-635) per sample and frame.  keys: per sample one key per point or None.
    -> (out_points_list, num_delta_points_list, per-sample list of the segments as (name, rows))"""
    max_pre = cfg.get('num_previous_frames', 4)
    outs, num_delta, segs_all = [], [], []
    for s in range(len(points)):
        pts, finds = points[s], pts_frame_inds[s]
        dev = pts.device
        cur_points = pts[finds == 0]
        pre_mask = (finds < 0) & (finds >= -max_pre)
        pre_points, pre_finds = pts[pre_mask], finds[pre_mask]
        pre_keys = keys[s][pre_mask] if keys is not None and keys[s] is not None else None
        frames = seed_info[s][:max_pre]
        num_pre_frames = len(frames)
        if 'crop_frames' in cfg:
            num_pre_frames = min(cfg['crop_frames'], num_pre_frames)
        segs, select = [], []
        for i in range(num_pre_frames):
            b = frames[i]['gt_bboxes_3d']
            b = torch.as_tensor(np.asarray(b.tensor if hasattr(b, 'tensor') else b), dtype=torch.float32).to(dev)
            if len(b) == 0:
                continue
            lab = torch.as_tensor(np.asarray(frames[i]['gt_labels_3d'])).to(dev).float()
            b = enlarged(b, cfg['extra_width'], lab)
            fmask = pre_finds == -i - 1
            this_points = pre_points[fmask]
            idx = crop_indices(this_points, b, cfg.get('max_crop_points', 0),
                               pre_keys[fmask] if (pre_keys is not None and cfg.get('crop_shuffle', False)) else None)
            if counters is not None:
                counters['frames'] = counters.get('frames', 0) + 1
            if idx.numel() == 0:
                continue
            rows = F.pad(this_points[idx], (0, 1), 'constant', float(-i - 1) / 10)
            select.append(rows)
            segs.append((f'crop{i}', rows))
        if len(select) == 0:
            old = F.pad(pre_points[1:200, :], (0, 1), 'constant', float(-num_pre_frames) / 10)
            segs.append(('fallback', old))
        else:
            old = torch.cat(select, 0)
        if cfg.get('disable_incremental', False):
            outs.append(old)
            segs_all.append(segs)
            continue
        num_base = cfg.get('num_base_frame', max_pre)
        base_mask = pre_finds >= -num_base

        def delta(cur, pre):
            if len(pre) > 0:
                return find_delta_points_by_voxelization(pre, cur, cfg['voxel_size'], cfg['point_cloud_range'])
            return cur.new_zeros((0, cur.size(1)))

        d = F.pad(delta(cur_points, pre_points[base_mask]), (0, 1), 'constant', 0)
        segs.append(('delta0', d))
        if cfg.get('max_age', 0) > 0:
            last = pre_finds == -1
            d1 = F.pad(delta(pre_points[last], pre_points[(~last) & base_mask]), (0, 1), 'constant', -0.1)
            segs.append(('delta1', d1))
            d = torch.cat([d, d1], 0)
        num_delta.append(len(d))
        outs.append(torch.cat([old, d], 0))
        segs_all.append(segs)
    return outs, num_delta, segs_all


def frame_transform(points, mat):
    """the stated order of sst_points_frame_transform_f32, elementwise in float32: ((x * m0 + y * m1) + z * m2) + m3 per row of
    the matrix; the other columns are copied"""
    m = torch.as_tensor(np.asarray(mat, np.float32)).to(points.device)
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    out = points.clone()
    for r in range(3):
        out[:, r] = ((x * m[r, 0] + y * m[r, 1]) + z * m[r, 2]) + m[r, 3]
    return out
