"""numpy / torch restatement of the CTRL test-time augmentation (sst_amd/tracklet_tta.py, csrc/tracklet_tta.hip), operation by
operation, written from the reference's sources: MultiScaleFlipAug3D's loop (mmdet3d/datasets/pipelines/test_time_aug.py:88-109),
TrackletGlobalRotScaleTrans (tracklet_pipelines.py:329-355) and TrackletRandomFlip (:414-439) in THAT order, PointsRangeFilter,
TrackletRoIHead.inverse_aug (mmdet3d/models/roi_heads/tracklet_roi_head.py:168-179), LiDARTracklet.update_from_prediction and
shared2ego (mmdet3d/core/bbox/structures/lidar_tracklet.py:403-493) and LiDARTracklet.merge_augs (:548-602).  The 2 x 2 rotation,
the range test, the shuffle keys and the frame matrices are tests/augment_ref.py's and tests/tracklet_augment_ref.py's: imported,
not copied.  tests/test_tracklet_tta_host.py pins this file to the reference's classes (tests/golden/tracklet_tta.npz);
tests/test_gpu_tracklet_tta.py pins the kernels to it."""
import os

import numpy as np
import torch

from augment_ref import F, PI32, in_range_3d, rotate_xy, shuffle_keys
from tracklet_augment_ref import pose_points

VIEW_SEED = np.uint64(0xD6E8FEB86659FD93)
PI = float(np.pi)
ROTS5 = [0, 2 * PI / 5, 4 * PI / 5, -4 * PI / 5, -2 * PI / 5]
# the cases of tests/golden/tracklet_tta.npz: the tracklet of make_tracklet_pipeline.make_inputs and MultiScaleFlipAug3D's arguments
GOLDEN_CASES = [dict(trk=0, flip=True, h=True, v=True, rots=0),                                        # the shipped configs: K = 4
                dict(trk=1, flip=True, h=True, v=True, rots=0),
                dict(trk=1, flip=False, h=True, v=True, rots=[0.3]),                                   # K = 1
                dict(trk=1, flip=True, h=True, v=False, rots=[0.0]),                                   # K = 2
                dict(trk=1, flip=False, h=False, v=False, rots=[PI / 2, 0, -PI / 2]),                   # K = 3
                dict(trk=2, flip=False, h=False, v=False, rots=ROTS5),                                  # K = 5
                dict(trk=1, flip=True, h=True, v=True, rots=ROTS5),                                     # K = 20
                dict(trk=1, flip=True, h=True, v=True, rots=[0.0, 0.4, -0.4, 1.1, -1.1, 2.0, -2.0, 3.0])]   # K = 32


def enumerate_views(flip, pcd_horizontal_flip, pcd_vertical_flip, pts_rots):
    """[(flip_h, flip_v, angle)] in the loop order of test_time_aug.py:88-109"""
    hs = [False, True] if flip and pcd_horizontal_flip else [False]
    vs = [False, True] if flip and pcd_vertical_flip else [False]
    rots = list(pts_rots) if isinstance(pts_rots, (list, tuple)) else [float(pts_rots)]
    return [(h, v, float(r)) for h in hs for v in vs for r in rots]


def angle_f32(angle):
    """-> (the float32 angle, its cos, its sin): ``tensor.new_tensor(angle)``, ``torch.cos`` / ``torch.sin`` on the CPU"""
    a = torch.tensor(float(angle), dtype=torch.float64).to(torch.float32)
    return F(a.item()), F(torch.cos(a).item()), F(torch.sin(a).item())


def view_points(xyz, view):
    """float32 [N, 3] -> the view's coordinates: rotation (BasePoints.rotate(-angle): x' = x cos + y sin, y' = x (-sin) + y cos),
    scale by 1, translation by +0.0 (the zero-std normal draw), flip h (y = -y), flip v (x = -x)"""
    h, v, angle = view
    _, c, s = angle_f32(angle)
    xyz = np.asarray(xyz, F).copy()
    xyz[:, 0], xyz[:, 1] = rotate_xy(xyz[:, 0].copy(), xyz[:, 1].copy(), c, s)
    with np.errstate(invalid='ignore', over='ignore'):
        xyz = ((xyz * F(1.0)).astype(F) + F(0.0)).astype(F)
    if h:
        xyz[:, 1] = -xyz[:, 1]
    if v:
        xyz[:, 0] = -xyz[:, 0]
    return xyz


def view_boxes(boxes, view):
    """float32 [n, 7] -> the view's boxes: rotate(angle), scale(1), translate(+0.0), flip h, flip v (lidar_box3d.py)"""
    h, v, angle = view
    a, c, s = angle_f32(angle)
    b = np.asarray(boxes, F).copy()
    b[:, 0], b[:, 1] = rotate_xy(b[:, 0].copy(), b[:, 1].copy(), c, s)
    with np.errstate(invalid='ignore', over='ignore'):
        b[:, 6] = b[:, 6] + a
        b[:, :6] = b[:, :6] * F(1.0)
        b[:, :3] = b[:, :3] + F(0.0)
        if h:
            b[:, 1] = -b[:, 1]
            b[:, 6] = -b[:, 6] + PI32
        if v:
            b[:, 0] = -b[:, 0]
            b[:, 6] = -b[:, 6]
    return b.astype(F)


def view_sample(frames, mats, deco, frame_values, view, k, point_range, shuffle, seed, sample):
    """view ``k`` of one sample: ``frames`` the per-frame [n_f, C] rows, ``mats`` [n, 4, 4] (or [n, 3, 4]), ``deco`` [n, D],
    ``frame_values`` int32 [n] -> (rows [M, C + D], frame values int32 [M], the input row of every output row)"""
    lens = np.array([f.shape[0] for f in frames], np.int64)
    cols = frames[0].shape[1] if len(frames) else 3
    rows = np.concatenate([np.asarray(f, F).reshape(-1, cols) for f in frames]) if len(frames) else np.zeros((0, cols), F)
    of = np.repeat(np.arange(len(frames)), lens)
    n = rows.shape[0]
    xyz = pose_points(rows[:, :3], np.asarray(mats, F)[of][:, :3, :]) if n else np.zeros((0, 3), F)
    xyz = view_points(xyz, view)
    keep = in_range_3d(xyz, point_range) if point_range is not None else np.ones(n, bool)
    idx = np.nonzero(keep)[0]
    if shuffle:
        with np.errstate(over='ignore'):
            folded = np.uint64(seed) + VIEW_SEED * np.uint64(k)
        idx = idx[np.argsort(shuffle_keys(folded, sample, n)[idx], kind='stable')]
    out = np.concatenate([xyz, rows[:, 3:], np.asarray(deco, F).reshape(len(frames), -1)[of]], 1)[idx]
    return out.astype(F), np.asarray(frame_values, np.int32)[of][idx], idx


def inverse_view(boxes, view):
    """inverse_aug on float32 [n, 7]: flip h undone, flip v undone, rotate(-angle) (cos and sin of the float32 -angle)"""
    h, v, angle = view
    b = np.asarray(boxes, F).copy()
    with np.errstate(invalid='ignore', over='ignore'):
        if h:
            b[:, 1] = -b[:, 1]
            b[:, 6] = -b[:, 6] + PI32
        if v:
            b[:, 0] = -b[:, 0]
            b[:, 6] = -b[:, 6]
        a, c, s = angle_f32(-float(angle_f32(angle)[0]))
        b[:, 0], b[:, 1] = rotate_xy(b[:, 0].copy(), b[:, 1].copy(), c, s)
        b[:, 6] = b[:, 6] + a
    return b.astype(F)


def ego_matrices(poses, shared_pose):
    """``torch.linalg.inv(stack(pose_list)) @ shared_pose`` in float32 -> [n, 4, 4] (shared2ego, lidar_tracklet.py:451-468)"""
    tgt = torch.as_tensor(np.asarray(poses), dtype=torch.float32)
    return (torch.linalg.inv(tgt) @ torch.as_tensor(np.asarray(shared_pose), dtype=torch.float32)).numpy()


def apply_poses(boxes, mm, einsum=True):
    """shared2ego's arithmetic on float32 [n, 7] with mm [n, 4, 4]: the centre by the full matrix, the heading (sin yaw, cos yaw,
    0) by its rotation, atan2.  ``einsum``: through torch.einsum as the reference does (bit for bit with it); otherwise the
    kernel's stated order ((m0 x + m1 y) + m2 z) + m3 and m0 sin + m1 cos, with torch's sin / cos / atan2"""
    src = torch.as_tensor(np.asarray(boxes, F))
    mm = torch.as_tensor(np.asarray(mm, F)).clone()
    yaw = src[:, 6]
    if einsum:
        center_h = torch.nn.functional.pad(src[:, :3], (0, 1), 'constant', 1)
        heading_h = torch.nn.functional.pad(torch.stack([torch.sin(yaw), torch.cos(yaw), torch.zeros_like(yaw)], 1), (0, 1), 'constant', 1)
        center = torch.einsum('nij,nj->ni', mm, center_h)[:, :3]
        mm[:, :3, 3] = 0
        heading = torch.einsum('nij,nj->ni', mm, heading_h)[:, :3]
        hx, hy = heading[:, 0], heading[:, 1]
    else:
        center = torch.as_tensor(pose_points(src[:, :3].numpy(), mm[:, :3, :].numpy()))
        sn, cs = torch.sin(yaw), torch.cos(yaw)
        hx = mm[:, 0, 0] * sn + mm[:, 0, 1] * cs
        hy = mm[:, 1, 0] * sn + mm[:, 1, 1] * cs
    return torch.cat([center, src[:, 3:6], torch.atan2(hx, hy)[:, None]], 1).numpy().astype(F)


def update_views(decoded, scores, valid, old_boxes, old_scores, mm, views, einsum=True):
    """per view inverse_aug and update_from_prediction: decoded [K, n, 7] float32, scores [K, n] float32, valid [K, n] bool,
    old_boxes [n, 7] float32 (un-augmented, shared pose), old_scores float64 [n] -> (ego boxes float32 [K, n, 7], scores float64
    [K, n]): the old box (through the same matrix) and the old score where the RoI was invalid"""
    old_ego = apply_poses(old_boxes, mm, einsum)
    out_b, out_s = [], []
    for k, view in enumerate(views):
        new = apply_poses(inverse_view(decoded[k], view), mm, einsum)
        m = np.asarray(valid[k], bool)
        out_b.append(np.where(m[:, None], new, old_ego))
        out_s.append(np.where(m, np.asarray(scores[k], F).astype(np.float64), np.asarray(old_scores, np.float64)))
    return np.stack(out_b).astype(F), np.stack(out_s).astype(np.float64)


def merge(all_boxes, all_scores, mode, iou_merge_thresh=None, iou_fn=None):
    """LiDARTracklet.merge_augs on all_boxes float32 [K, n, 7] and all_scores float64 [K, n] -> (boxes float64 [n, 7], scores
    float64 [n], the scores the merge used [K, n]).  ``iou_fn``: ([n, 7], [n, 7]) float32 -> [n] float32 aligned 3-D IoU"""
    all_boxes = np.asarray(all_boxes, F)
    all_scores = np.asarray(all_scores, np.float64).copy()
    num_augs, len_trk = all_scores.shape
    with np.errstate(invalid='ignore', divide='ignore'):
        if mode == 'max':
            argmax = all_scores.argmax(0)
            return all_boxes[argmax, range(len_trk), :].astype(np.float64), all_scores[argmax, range(len_trk)], all_scores
        if mode == 'iou_clamped_weighted':
            flat = all_boxes.reshape(num_augs * len_trk, 7)
            base = np.concatenate([all_boxes[0]] * num_augs, 0)
            ious = np.asarray(iou_fn(base, flat), F).reshape(num_augs, len_trk).copy()
            ious[0, :] = 1
            all_scores *= (ious > F(iou_merge_thresh)).astype(np.float64)
        elif mode != 'weighted':
            raise KeyError(mode)
        box_6dim = (all_boxes[..., :6] * all_scores[..., None]).sum(0) / all_scores.sum(0)[:, None]
        median_yaw = np.median(all_boxes[..., 6], 0)
        return np.concatenate([box_6dim, median_yaw[:, None]], 1), all_scores.mean(0), all_scores


def load_golden(golden_dir):
    with np.load(os.path.join(golden_dir, 'tracklet_tta.npz'), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def golden_case(g, c):
    """case ``c`` of the golden: everything stored under ``c{c}_`` with the prefix removed, the per-frame points as a list"""
    pre = f'c{c}_'
    r = {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}
    r['frames'] = np.split(r['points'], np.cumsum(r['frame_lens'])[:-1]) if len(r['frame_lens']) else []
    r['views'] = [(bool(h), bool(v), float(a)) for h, v, a in r['view_table']]
    return r
