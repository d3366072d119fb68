"""CTRL's offline stage (csrc/tracklet_prep.hip, sst_amd/tracklet_prep.py) restated on the CPU the way the reference's tools/ctrl/
scripts compute it - pair by pair, frame by frame, box by box: for tests/test_tracklet_prep_host.py,
tests/test_gpu_tracklet_prep.py, tests/golden/make_tracklet_prep.py and tools/tracklet_prep_bench.py.

- max_iou / affinity / candidates / stats: generate_candidates.py:39-78 with LiDARTracklet.max_iou (lidar_tracklet.py:210-229); the
  IoU is tracklet_ref.aligned_iou, which goes through tests/box_ops_ref.py.
- membership / crops / counts / keep_masks: generate_track_input.py:88-101 and remove_empty.py:82-134 (box_grouping, group_size 1);
  the inside test is oracle.point_pool_oracle's restatement of points_in_boxes_cpu.cpp, the one the point pool and box ops tests use.
- enlarged_box / enlarged_box_hw / to_bottom_centre: lidar_box3d.py:269-285, :331-346 and base_box3d.py:62-65 in float32 (or float64).
"""
import os

import numpy as np
import torch

import tracklet_ref as T
from oracle import point_pool_oracle as O

TS0 = T.TS0
HERE = os.path.dirname(os.path.abspath(__file__))
CONFIG_DIR = os.path.join(HERE, 'golden', 'configs', 'ctrl_data')


def data_config(name='fsd_base_vehicle'):
    """one of the reference's tools/ctrl/data_configs/*.yaml (fixtures under tests/golden/configs/ctrl_data)"""
    import yaml
    with open(os.path.join(CONFIG_DIR, name + '.yaml')) as f:
        return yaml.safe_load(f)


class Trk(T.Trk):
    """the fields of a tracklet the offline stage reads"""

    def __init__(self, boxes, ts_list, score_list, type_, segment_name, id_, in_world=True):
        super().__init__(boxes, ts_list, score_list, type_)
        self.segment_name, self.id, self.in_world = segment_name, id_, in_world

    def __len__(self):
        return len(self.ts_list)


def lidar(trk, device=None):
    """-> the library's frozen LiDARTracklet of a Trk"""
    import sst_amd
    t = sst_amd.LiDARTracklet(trk.segment_name, trk.id, int(trk.type), trk.in_world, trk.boxes.clone(), list(trk.ts_list),
                              list(trk.score_list))
    t.freeze()
    return t.to(device) if device is not None else t


# ---- affinity -------------------------------------------------------------------------------------------------------------------

def shared(a, b):
    ib = {ts: i for i, ts in enumerate(b.ts_list)}
    pairs = [(i, ib[ts]) for i, ts in enumerate(a.ts_list) if ts in ib]
    return [i for i, _ in pairs], [j for _, j in pairs]


def max_iou(pd, gt, dtype=torch.float32, iou_fn=None):
    """LiDARTracklet.max_iou: 0 without a shared timestamp, else the maximum (torch.max: a NaN wins) of aligned_iou_3d"""
    assert pd.in_world == gt.in_world
    i1, i2 = shared(pd, gt)
    if not i1:
        return 0.0
    fn = iou_fn or (lambda x, y: T.aligned_iou(x, y, dtype))
    return fn(pd.boxes[i1], gt.boxes[i2]).max().item()


def affinity(trks_pd, trks_gt, dtype=torch.float32, iou_fn=None):
    """tracklet_assign's pair loop -> per predicted tracklet (gt indices, affinities); empty without ground truth in the segment"""
    by_seg = {}
    for i, t in enumerate(trks_gt):
        by_seg.setdefault(t.segment_name, []).append(i)
    npdt = np.float32 if dtype == torch.float32 else np.float64
    out = []
    for pd in trks_pd:
        idx = by_seg.get(pd.segment_name, [])
        out.append((np.asarray(idx, np.int64), np.asarray([max_iou(pd, trks_gt[i], dtype, iou_fn) for i in idx], npdt).reshape(-1)))
    return out


def candidates(aff, thresh):
    """-> per predicted tracklet the indices (into the ground-truth list) with affinity > thresh, in ground-truth order"""
    return [[int(g) for g, v in zip(idx, a) if float(v) > thresh] for idx, a in aff]


def stats(lens, cands):
    """``stats`` of generate_candidates.py:71-77 -> (tracklet FP rate, box FP rate)"""
    unmatched = [n for n, c in zip(lens, cands) if len(c) == 0]
    return len(unmatched) / len(lens), sum(unmatched) / sum(lens)


# ---- box modifications ------------------------------------------------------------------------------------------------------------

def enlarged_box(boxes, extra_width):
    b = np.array(boxes, copy=True)
    dt = b.dtype.type
    b[:, 3:6] += dt(extra_width * 2)
    b[:, 2] -= dt(extra_width)
    if extra_width < 0:
        bad = (b[:, 3:6] <= 0).any(1)
        b[bad] = np.asarray(boxes)[bad]
    return b


def enlarged_box_hw(boxes, extra_width):
    b = np.array(boxes, copy=True)
    b[:, 3:5] += b.dtype.type(extra_width * 2)
    if extra_width < 0:
        bad = (b[:, 3:5] <= 0).any(1)
        b[bad] = np.asarray(boxes)[bad]
    return b


def to_bottom_centre(boxes, origin):
    b = np.array(boxes, copy=True)
    dt = b.dtype.type
    if tuple(origin) != (0.5, 0.5, 0):
        b[:, :3] += b[:, 3:6] * (np.asarray((0.5, 0.5, 0), b.dtype) - np.asarray(origin, b.dtype))
    return b.astype(dt)


# ---- membership and crops -----------------------------------------------------------------------------------------------------------

def membership(boxes, pts):
    """[B, N] bool: point n inside box b, every box alone (oracle.point_pool_oracle: float32 operation by operation)"""
    r = np.asarray(boxes, np.float32).reshape(-1, 7)
    p = np.asarray(pts, np.float32)[:, :3]
    if len(r) == 0 or len(p) == 0:
        return np.zeros((len(r), len(p)), bool)
    lx, ly, lz = O.local_coords(r, p)
    return O.inside(lx, ly, lz, r[:, 3], r[:, 4], r[:, 5])


def membership_f64(boxes, pts):
    """the same test in float64 (the golden's second run)"""
    r = np.asarray(boxes, np.float64).reshape(-1, 7)
    p = np.asarray(pts, np.float64)[:, :3]
    cz = r[:, 2] + r[:, 5] * 0.5
    rot = r[:, 6] + np.pi / 2
    sx, sy = p[None, :, 0] - r[:, None, 0], p[None, :, 1] - r[:, None, 1]
    lx = sx * np.cos(rot)[:, None] + sy * (-np.sin(rot))[:, None]
    ly = sx * np.sin(rot)[:, None] + sy * np.cos(rot)[:, None]
    lz = p[None, :, 2] - cz[:, None]
    return O.inside(lx, ly, lz, r[:, 3], r[:, 4], r[:, 5])


def face_clearance(boxes, pts):
    """[B, N] distance of every point to the nearest face plane of every box"""
    if len(boxes) == 0 or len(pts) == 0:
        return np.full((len(boxes), len(pts)), np.inf)
    return O.face_clearance(np.asarray(boxes, np.float32), np.asarray(pts, np.float32)[:, :3], np.zeros(3, np.float32))


def crops(points_list, boxes_list, member=membership):
    """-> (rows, src, counts) in (frame, box, ascending point index) order: pc[inbox_inds == 0] of every box of every frame"""
    rows, src, counts = [], [], []
    cols = points_list[0].shape[1] if points_list else 3
    for p, b in zip(points_list, boxes_list):
        m = member(b, p)
        for k in range(len(b)):
            idx = np.nonzero(m[k])[0]
            rows.append(np.asarray(p)[idx])
            src.append(idx.astype(np.int64))
            counts.append(len(idx))
    rows = np.concatenate(rows + [np.zeros((0, cols), np.float32)], 0)
    return rows, np.concatenate(src + [np.zeros(0, np.int64)]), np.asarray(counts, np.int32).reshape(-1)


def crop_tracklets(trks, frames, extra_width, member=membership):
    """extract_and_save_point for the tracklets of one segment -> per tracklet its pc_list"""
    pcs = [[] for _ in trks]
    for ts in sorted(frames):
        for i, t in enumerate(trks):
            if ts not in t.ts_list:
                continue
            k = t.ts_list.index(ts)
            assert k == len(pcs[i])
            box = enlarged_box(t.boxes[k:k + 1].numpy(), extra_width)
            pcs[i].append(np.asarray(frames[ts])[member(box, frames[ts])[0]])
    return pcs


def keep_masks(boxes_list, points_list, bottom_lift, extra_hw=None, origin=(0.5, 0.5, 0.5), member=membership):
    """process_single_frame with box_grouping and group_size 1 -> (masks, dropped)"""
    masks = []
    for b, p in zip(boxes_list, points_list):
        b = to_bottom_centre(np.asarray(b, np.float32), origin)
        b[:, 2] += b[:, 5] * np.float32(bottom_lift)
        if extra_hw is not None:
            b = enlarged_box_hw(b, extra_hw)
        masks.append(member(b, p).any(1))
    return masks, [not bool(m.any()) for m in masks]


# ---- scenes ---------------------------------------------------------------------------------------------------------------------

def frames_ts(idx):
    return [TS0 + 100_000 * int(i) for i in idx]


def gold_scene(g):
    """the tracklets of tests/golden/tracklet_prep.npz -> (predicted, ground truth) lists of Trk"""
    out = []
    for tag in ('pd', 'gt'):
        trks, r0 = [], 0
        for k, n in enumerate(g[f'{tag}_lens'].tolist()):
            trks.append(Trk(g[f'{tag}_boxes'][r0:r0 + n], g[f'{tag}_ts'][r0:r0 + n].tolist(), g[f'{tag}_scores'][r0:r0 + n].tolist(),
                            int(g[f'{tag}_types'][k]), str(g[f'{tag}_segs'][k]), f'{tag}{k}'))
            r0 += n
        out.append(trks)
    return out


def gold_crop_scene(g):
    """-> (tracklets, frames {ts: points}) of the golden's crop case"""
    trks, r0 = [], 0
    for k, n in enumerate(g['crop_lens'].tolist()):
        trks.append(Trk(g['crop_boxes'][r0:r0 + n], g['crop_ts'][r0:r0 + n].tolist(), [0.5] * n, 1, 'segA', f'c{k}'))
        r0 += n
    frames, p0 = {}, 0
    for ts, n in zip(g['crop_frame_ts'].tolist(), g['crop_frame_lens'].tolist()):
        frames[int(ts)] = g['crop_points'][p0:p0 + n]
        p0 += n
    return trks, frames


def split(flat, lens):
    out, k = [], 0
    for n in lens:
        out.append(flat[k:k + int(n)])
        k += int(n)
    return out


def points_around(rng, boxes, n_in, n_bg, cols, margin=1e-3):
    """n_in points drawn inside (or just around) randomly chosen boxes + n_bg background points, [n, cols] float32; points within
    ``margin`` of a face plane of any box are pushed out of the scene's way (re-drawn)"""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 7)
    pts = []
    if len(boxes) and n_in:
        k = rng.integers(0, len(boxes), n_in)
        b = boxes[k]
        loc = rng.uniform(-0.75, 0.75, (n_in, 3)) * b[:, [4, 3, 5]]        # local x along l, y along w
        rot = b[:, 6].astype(np.float64) + np.pi / 2
        cs, sn = np.cos(rot), np.sin(rot)
        # the inverse of local_coords: lx = sx cos - sy sin, ly = sx sin + sy cos
        sx = loc[:, 0] * cs + loc[:, 1] * sn
        sy = -loc[:, 0] * sn + loc[:, 1] * cs
        pts.append(np.stack([b[:, 0] + sx, b[:, 1] + sy, b[:, 2] + b[:, 5] * 0.5 + loc[:, 2]], 1))
    if n_bg:
        pts.append(rng.uniform(-1, 1, (n_bg, 3)) * np.array([40.0, 40.0, 3.0]))
    xyz = np.concatenate(pts + [np.zeros((0, 3))], 0).astype(np.float32)
    rng.shuffle(xyz)
    for _ in range(50):
        bad = (face_clearance(boxes, xyz) < margin).any(0) if len(boxes) and len(xyz) else np.zeros(len(xyz), bool)
        if not bad.any():
            break
        xyz[bad] += rng.normal(0, 0.05, (int(bad.sum()), 3)).astype(np.float32)
    else:
        raise RuntimeError('points too close to a face')
    extra = rng.uniform(0, 1, (len(xyz), cols - 3)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([xyz, extra], 1))
