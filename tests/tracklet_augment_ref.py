"""Float32 numpy restatement of the CTRL tracklet pipeline (sst_amd/tracklet_augment.py, csrc/tracklet_augment.hip), operation by
operation, written from the reference's sources: mmdet3d/datasets/pipelines/tracklet_pipelines.py (TrackletCutting :105-138,
TrackletPoseTransform :149-208, PointDecoration :455-506, TrackletRandomFlip :414-439, TrackletGlobalRotScaleTrans :329-355,
TrackletNoise :550-562) and mmdet3d/core/bbox/structures/lidar_tracklet.py:106-118, :495-546.  The flips, the rotation, the
scale, the translation, the range test, the shuffle keys and the box transforms are tests/augment_ref.py's: imported, not copied.
tests/test_tracklet_augment_host.py pins this file to the reference's classes (tests/golden/tracklet_pipeline.npz);
tests/test_gpu_tracklet_augment.py pins the kernels to it bit by bit."""
import os

import numpy as np

from augment_ref import (F, flip_boxes, flip_points, in_range_3d, rotate_boxes, rotate_points, scale_boxes,  # noqa: F401
                         scale_points, shuffle_keys, transform_boxes, transform_points, translate_boxes, translate_points)

DECO_WIDTH = dict(yaw=1, size=3, score=1, length=1)


def cut_frames(length, head, tail):
    """the frames TrackletCutting keeps -> their indices before the cut, which are also the values pts_frame_inds keeps"""
    return np.arange(head, length - tail, dtype=np.int32)


def cutting_draws(length, cfg, rng):
    """TrackletCutting's decision (min_length, ratio, max_cut_ratio, max_length) with the reference's draws -> (head, tail)"""
    min_length, ratio, max_cut_ratio, max_length = cfg
    if length < min_length or (rng.rand() > ratio and length < max_length):
        return 0, 0
    cut_len = length - max_length if length > max_length else int(length * max_cut_ratio * rng.rand())
    if cut_len < 1:
        return 0, 0
    head = int(rng.randint(0, cut_len))
    return head, cut_len - head


def noise_boxes(boxes, u_center=None, max_center=None, u_size=None, max_size=None, u_yaw=None, max_yaw=None):
    """add_center_noise / add_size_noise / add_yaw_noise: noise = ((u - 0.5) * 2) * max, every operation in float32; u of shape
    [n, 3] / [n] or, when consistent, [3] / [1]"""
    b = np.asarray(boxes, F).copy()
    if b.shape[0] == 0:
        return b
    if u_center is not None:
        b[:, :3] = b[:, :3] + ((np.asarray(u_center, F) - F(0.5)) * F(2)) * np.asarray(max_center, F)
    if u_size is not None:
        b[:, 3:6] = b[:, 3:6] * (F(1) + ((np.asarray(u_size, F) - F(0.5)) * F(2)) * np.asarray(max_size, F))
    if u_yaw is not None:
        b[:, 6] = b[:, 6] + ((np.asarray(u_yaw, F) - F(0.5)) * F(2)) * F(max_yaw)
    return b.astype(F)


def decoration(boxes, scores, properties, length):
    """float32 [n, D]: yaw = float32(double(yaw) / 3.1415), size = float32 size / float32 10, score = float32(score),
    length = float32(len / 100)"""
    b = np.asarray(boxes, F)
    n = b.shape[0]
    cols = []
    for pro in properties:
        if pro == 'yaw':
            cols.append((b[:, 6].astype(np.float64) / 3.1415).astype(F)[:, None])
        elif pro == 'size':
            cols.append((b[:, 3:6] / F(10)).astype(F))
        elif pro == 'score':
            cols.append(np.asarray(scores, np.float64).astype(F).reshape(n, 1))
        elif pro == 'length':
            cols.append(np.full((n, 1), length / 100, np.float64).astype(F))
        else:
            raise KeyError(pro)
    return np.concatenate(cols, 1) if cols else np.zeros((n, 0), F)


def pose_points(xyz, m):
    """x' = ((m00 x + m01 y) + m02 z) + m03 and likewise y', z': rows 0..2 of the frame's 4 x 4 matrix, float32, every product
    and sum rounded on its own.  ``m`` [4, 4] or [3, 4], or one matrix per point [N, 3 | 4, 4]"""
    xyz = np.asarray(xyz, F)
    m = np.asarray(m, F)
    m = np.broadcast_to(m, (xyz.shape[0],) + m.shape[-2:]) if m.ndim == 2 else m
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(invalid='ignore', over='ignore'):
        out = [((m[:, k, 0] * x + m[:, k, 1] * y) + m[:, k, 2] * z) + m[:, k, 3] for k in range(3)]
    return np.stack(out, 1).astype(F)


def augment_sample(frames, mats, deco, frame_values, rec, sample):
    """one sample: ``frames`` the kept frames' [n_f, C] rows, ``mats`` [n, 4, 4] (or [n, 3, 4]), ``deco`` [n, D], ``frame_values``
    int32 [n], ``rec`` the sample's record -> (rows [M, C + D], frame values int32 [M], the input row of every output row)"""
    lens = np.array([f.shape[0] for f in frames], np.int64)
    cols = frames[0].shape[1] if len(frames) else 3
    rows = np.concatenate([np.asarray(f, F).reshape(-1, cols) for f in frames]) if len(frames) else np.zeros((0, cols), F)
    of = np.repeat(np.arange(len(frames)), lens)
    n = rows.shape[0]
    xyz = pose_points(rows[:, :3], np.asarray(mats, F)[of][:, :3, :]) if n else np.zeros((0, 3), F)
    xyz = transform_points(xyz, rec)
    keep = in_range_3d(xyz, rec['range'])
    idx = np.nonzero(keep)[0]
    if rec['shuffle']:
        idx = idx[np.argsort(shuffle_keys(rec['seed'], sample, n)[idx], kind='stable')]
    out = np.concatenate([xyz, rows[:, 3:], np.asarray(deco, F).reshape(len(frames), -1)[of]], 1)[idx]
    return out.astype(F), np.asarray(frame_values, np.int32)[of][idx], idx


def load_golden(golden_dir):
    with np.load(os.path.join(golden_dir, 'tracklet_pipeline.npz')) as z:
        return {k: z[k] for k in z.files}


def golden_case(g, t):
    """tracklet ``t`` of the golden: everything stored under ``t{t}_`` with the prefix removed, the per-frame points as a list"""
    pre = f't{t}_'
    r = {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}
    r['frames'] = np.split(r['points'], np.cumsum(r['frame_lens'])[:-1]) if len(r['frame_lens']) else []
    r['cands'] = []
    for c in range(int(r['n_cands'])):
        cp = f'c{c}_'
        r['cands'].append({k[len(cp):]: v for k, v in r.items() if k.startswith(cp)})
    return r
