"""The CTRL tracklet family's data structure and training targets: LiDARTracklet (core/bbox/structures/lidar_tracklet.py as far
as training and simple_test use it), TrackletAssigner (core/bbox/assigners/tracklet_assigner.py), the fused targets of a whole
batch of tracklets (TrackletRoIHead._select_one2one_candidates / _assign_and_sample and FullySparseBboxHead.get_targets in one
launch, nothing read back) and the input rows of the box head (tracklet_roi_head.py:247-258, one launch forward and one
backward).  The work runs in csrc/tracklet.hip behind the C ABI of include/sst_amd.h; there is no CPU path.

A tracklet holds its boxes as ONE [n, 7] tensor (``boxes``); ``box_list`` is the list of its [1, 7] row views, so ``to(device)``
is one copy where the reference moves a list of 1 x 7 tensors one by one.
"""
import copy
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from . import box_ops
from ._head_common import cfg_get as _cfg_get

MAX_CLASSES = 16

REFUSED_METHODS = ('merge_augs', 'extend', 'extend_all', 'add_center_noise', 'add_size_noise', 'add_yaw_noise',
                   'random_frame_drop')


def _refuse(name):
    raise NotImplementedError(f'sst_amd.LiDARTracklet.{name}: part of the reference\'s data pipeline (Tracklet* transforms, '
                              f'test-time augmentation), which this library does not build')


def aligned_iou_3d(boxes1, boxes2):
    """LiDARInstance3DBoxes.aligned_iou_3d (lidar_box3d.py:404-450) of [N, 7] x [N, 7] device boxes -> [N]: the aligned BEV
    overlap of the box ops x the clamped height overlap over the clamped union of the volumes.  The tracklet targets kernel
    produces these values bit for bit."""
    a, b = boxes1[:, :7], boxes2[:, :7]
    if a.size(0) == 0:
        return a.new_zeros((0,))
    bev = box_ops.boxes_overlap_1to1(box_ops.xywhr2xyxyr(box_ops.lidar_bev(a)).contiguous(),
                                     box_ops.xywhr2xyxyr(box_ops.lidar_bev(b)).contiguous())
    overlaps_h = torch.clamp(torch.min(a[:, 2] + a[:, 5], b[:, 2] + b[:, 5]) - torch.max(a[:, 2], b[:, 2]), min=0)
    overlaps_3d = bev * overlaps_h
    volume1, volume2 = a[:, 3] * a[:, 4] * a[:, 5], b[:, 3] * b[:, 4] * b[:, 5]
    return overlaps_3d / torch.clamp(volume1 + volume2 - overlaps_3d, min=1e-8)


def _heading_unit_vector(boxes):
    """BaseInstance3DBoxes.heading_unit_vector as frame_transform / shared2ego read it back with atan2(v[0], v[1]): the yaw of a
    LiDAR box is measured from the y axis (the coordinate convention of the reference's 0.x box class)"""
    yaw = boxes[:, 6]
    return torch.stack([torch.sin(yaw), torch.cos(yaw), torch.zeros_like(yaw)], 1)


class LiDARTracklet(object):
    """core/bbox/structures/lidar_tracklet.py: the boxes, timestamps and scores of one object over the frames of a segment."""

    type_mapping = {1: 'Car', 2: 'Pedestrian', 4: 'Cyclist'}
    list_fields = ['box_list', 'score_list', 'ts_list', 'pose_list']

    def __init__(self, seg_name, id_, type_, in_world, box_list=None, ts_list=None, score_list=None, num_pts_in_boxes=None):
        assert isinstance(type_, int)
        assert isinstance(id_, str)
        self.ts_list = [] if box_list is None else list(ts_list)
        self.score_list = [] if box_list is None else list(score_list)
        self._set_boxes(box_list)
        self.pc_list = []
        self.num_pts_in_boxes = num_pts_in_boxes
        self.segment_name = seg_name
        self.id = id_
        self.type = type_
        self.set_uuid()
        self.frozen = False
        self.in_world = in_world
        self.type_format = 'waymo'

    # ---- storage: one [n, 7] tensor, box_list = its [1, 7] row views ---------------------------------------------------

    def _set_boxes(self, boxes):
        """boxes: None, an [n, 7 | 9] tensor / array, or a list of [1, 7] (or [7]) tensors / arrays / box objects"""
        if boxes is None or (isinstance(boxes, (list, tuple)) and len(boxes) == 0):
            dev = getattr(self, 'device', 'cpu')
            self.boxes = torch.zeros((0, 7), dtype=torch.float32, device=dev)
        elif torch.is_tensor(boxes):
            self.boxes = boxes.reshape(-1, boxes.size(-1)).to(torch.float32)
        elif isinstance(boxes, np.ndarray):
            self.boxes = torch.as_tensor(boxes.reshape(-1, boxes.shape[-1]), dtype=torch.float32)
        else:
            rows = [b.tensor if hasattr(b, 'tensor') else torch.as_tensor(b) for b in boxes]
            self.boxes = torch.cat([r.reshape(1, -1).to(torch.float32) for r in rows], 0)
        self.size = self.boxes.size(0)

    @property
    def box_list(self):
        return [self.boxes[i:i + 1] for i in range(self.boxes.size(0))]

    @box_list.setter
    def box_list(self, value):
        self._set_boxes(value)

    def set_uuid(self):
        self.uuid = self.segment_name + '__' + self.id + '__' + str(self.type)

    def new_empty(self):
        empty = LiDARTracklet(self.segment_name, self.id + '_empty', self.type, self.in_world)
        empty.device = self.device
        empty.dtype = self.dtype
        empty.boxes = empty.boxes.to(self.device)
        empty.ts2index, empty.ts_set, empty.frozen = {}, set(), True
        if hasattr(self, 'type_name'):
            empty.type_name = self.type_name
        empty.type_format = self.type_format
        return empty

    def set_type(self, type, format):
        self.type = type
        self.type_format = format

    def set_type_name(self):
        assert self.type_format == 'waymo'
        self.type_name = self.type_mapping[self.type]

    def append(self, box, score, ts, in_world):
        row = (box.tensor if hasattr(box, 'tensor') else torch.as_tensor(box)).reshape(1, -1).to(self.boxes)
        self.boxes = torch.cat([self.boxes, row], 0) if self.boxes.size(0) else row
        self.ts_list.append(ts)
        self.score_list.append(score)
        self.size += 1
        assert self.in_world == in_world

    def freeze(self):
        self.ts2index = {ts: i for i, ts in enumerate(self.ts_list)}
        self.ts_set = set(self.ts_list)
        assert self.ts_list == sorted(self.ts_list)
        assert len(self.ts2index) == len(self.ts_list)
        assert self.boxes.size(0) == len(self.ts_list) == len(self.score_list)
        self.frozen = True
        self.device = self.boxes.device
        self.dtype = self.boxes.dtype
        self.size = len(self.ts_list)

    def remove(self, ts_list):
        """drop the frames with these timestamps (lidar_tracklet.py:106-118): ``list_fields`` and ``boxes`` keep the others in
        their order, the tracklet is frozen again -> keep_idx, the kept frames' former indices"""
        keep_ts = self.ts_set - set(ts_list if ts_list is not None else [])
        keep_idx = sorted(self.ts2index[ts] for ts in keep_ts)
        for f in self.list_fields:
            if f != 'box_list' and getattr(self, f, None) is not None:
                attr = getattr(self, f)
                setattr(self, f, [attr[i] for i in keep_idx])
        self.boxes = self.boxes[torch.as_tensor(keep_idx, dtype=torch.long, device=self.boxes.device)]
        self.freeze()
        return keep_idx

    # ---- dump / collate formats ----------------------------------------------------------------------------------------

    def to_dump_format(self):
        boxes = [b.cpu().numpy() for b in self.box_list]
        return (self.segment_name, self.id, self.type, self.in_world, boxes, self.ts_list, self.score_list, self.num_pts_in_boxes)

    @classmethod
    def from_dump_format(cls, input):
        input = copy.deepcopy(input)
        trk = cls(*input)
        trk.freeze()
        return trk

    def to_collate_format(self):
        """numpy in place of tensors (the reference's DataContainer collate): ``boxes`` becomes an [n, 7] array"""
        self.boxes = self.boxes.cpu().numpy()
        if getattr(self, 'pose_list', None) is not None:
            self.pose_list = [p.numpy() for p in self.pose_list]
        if getattr(self, 'shared_pose', None) is not None:
            self.shared_pose = self.shared_pose.numpy()

    def from_collate_format(self):
        self._set_boxes(self.boxes)
        if getattr(self, 'pose_list', None) is not None:
            self.pose_list = [torch.from_numpy(p) for p in self.pose_list]
        if getattr(self, 'shared_pose', None) is not None:
            self.shared_pose = torch.from_numpy(self.shared_pose)

    # ---- access ----------------------------------------------------------------------------------------------------------

    def __getitem__(self, key):
        assert isinstance(key, int)
        if key > 1e10:      # a timestamp
            i = self.ts2index.get(key)
            return None if i is None else self.boxes[i:i + 1]
        if key < self.size:
            return self.boxes[key:key + 1]
        raise KeyError

    def __len__(self):
        return self.size

    def ts_intersection(self, trk, return_sorted=True):
        inter = self.ts_set.intersection(trk.ts_set)
        return sorted(list(inter)) if return_sorted else inter

    def ts_iou(self, trk_b):
        """the share of the two tracklets' timestamps that both have (lidar_tracklet.py:202-208)"""
        sa, sb = set(self.ts_list), set(trk_b.ts_list)
        union = len(sa.union(sb))
        assert union > 0
        return len(sa.intersection(sb)) / union

    def max_iou(self, trk):
        """the largest aligned_iou_3d over the shared timestamps, 0 without one (lidar_tracklet.py:210-229) -> a Python float:
        the affinity kernel of sst_amd.tracklet_prep on this one pair (tracklet_affinity runs it on every pair of a segment)"""
        assert self.in_world == trk.in_world
        from . import tracklet_prep
        dev = tracklet_prep._device(None, [self.boxes, trk.boxes])
        return float(tracklet_prep._affinity_launch([self], [trk], [(0, 1)], dev)[0].item())

    def append_pc(self, pc, ts=None):
        """lidar_tracklet.py:70-74: the points of the next frame, in the order of ts_list"""
        assert self.frozen
        if ts is not None:
            assert ts == self.ts_list[len(self.pc_list)]
        self.pc_list.append(pc)

    def free_pc(self):
        self.pc_list = None

    def get_index_from_ts(self, ts):
        assert self.frozen
        return self.ts2index.get(ts, -1)

    def intersection_ious(self, trk):
        inter = self.ts_intersection(trk)
        if len(inter) == 0:
            return self.boxes.new_zeros(0)
        dev = self.boxes.device
        i1 = torch.tensor([self.ts2index[ts] for ts in inter], dtype=torch.long).to(dev, non_blocking=True)
        i2 = torch.tensor([trk.ts2index[ts] for ts in inter], dtype=torch.long).to(dev, non_blocking=True)
        return aligned_iou_3d(self.boxes[i1], trk.boxes.to(dev)[i2])

    def self_ious(self, trk):
        inter = self.ts_intersection(trk)
        out_ious = self.boxes.new_zeros(len(self))
        if len(inter) == 0:
            return out_ious
        inds = torch.tensor([self.ts2index[ts] for ts in inter], dtype=torch.long).to(self.boxes.device, non_blocking=True)
        out_ious[inds] = self.intersection_ious(trk)
        return out_ious

    def concated_boxes(self):
        """-> [n, 7] tensor (the reference wraps it in LiDARInstance3DBoxes; ``.tensor`` of that is this)"""
        return self.boxes

    def concated_scores(self):
        return torch.tensor(self.score_list, dtype=torch.float).reshape(-1).to(self.device, non_blocking=True)

    def concated_labels(self):
        return torch.full((len(self),), self.type, device=self.device, dtype=torch.long)

    def concated_boxes_from_ts(self, ts_list):
        if len(self) == 0:
            return (torch.zeros((len(ts_list), 7), device=self.device, dtype=self.dtype),
                    torch.zeros((len(ts_list),), device=self.device, dtype=torch.bool))
        idx = [self.ts2index.get(ts, -1) for ts in ts_list]
        idx_t = torch.tensor(idx, dtype=torch.long).to(self.device, non_blocking=True)
        mask = idx_t >= 0
        out = self.boxes[idx_t.clamp(min=0)] * mask[:, None].to(self.boxes.dtype)
        return out, mask

    def set_poses(self, ts2poses):
        self.pose_list = [ts2poses[ts] for ts in self.ts_list]

    # ---- geometry --------------------------------------------------------------------------------------------------------

    def flip(self, direction='horizontal'):
        """LiDARInstance3DBoxes.flip per box (lidar_box3d.py): horizontal mirrors y, vertical mirrors x"""
        assert direction in ('horizontal', 'vertical')
        if direction == 'horizontal':
            self.boxes[:, 1::7] = -self.boxes[:, 1::7]
            self.boxes[:, 6] = -self.boxes[:, 6] + np.pi
        else:
            self.boxes[:, 0::7] = -self.boxes[:, 0::7]
            self.boxes[:, 6] = -self.boxes[:, 6]

    def translate(self, trans):
        trans = torch.as_tensor(trans, dtype=self.boxes.dtype, device=self.boxes.device)
        self.boxes[:, :3] += trans

    def translate_by_ts(self, ts_list, movements):
        assert len(ts_list) == len(movements)
        for i, ts in enumerate(ts_list):
            if ts in self.ts2index:
                k = self.ts2index[ts]
                self.boxes[k, :3] += torch.as_tensor(movements[i], dtype=self.boxes.dtype, device=self.boxes.device)

    def scale(self, scale):
        self.boxes[:, :6] *= scale
        if self.boxes.size(1) > 7:
            self.boxes[:, 7:] *= scale

    def rotate(self, angle):
        """LiDARInstance3DBoxes.rotate per box with a scalar angle (lidar_box3d.py): centres by the matrix
        [[cos, -sin, 0], [sin, cos, 0], [0, 0, 1]] applied from the right, the yaw raised by the angle"""
        angle = torch.as_tensor(angle, dtype=self.boxes.dtype, device=self.boxes.device)
        rot_sin, rot_cos = torch.sin(angle), torch.cos(angle)
        rot_mat_T = self.boxes.new_tensor([[rot_cos, -rot_sin, 0], [rot_sin, rot_cos, 0], [0, 0, 1]])
        self.boxes[:, :3] = self.boxes[:, :3] @ rot_mat_T
        self.boxes[:, 6] += angle
        if self.boxes.size(1) == 9:
            self.boxes[:, 7:9] = self.boxes[:, 7:9] @ rot_mat_T[:2, :2]

    def frame_transform(self, pose, src_boxes=None, src_poses=None):
        """every box from its own frame's pose to ``pose`` (lidar_tracklet.py:348-387), all boxes in one batched product"""
        boxes = self.boxes if src_boxes is None else torch.cat([(b.tensor if hasattr(b, 'tensor') else b).reshape(1, -1)
                                                                  for b in src_boxes], 0)
        src_poses = self.pose_list if src_poses is None else src_poses
        assert getattr(self, 'shared_pose', None) is None
        mm = torch.linalg.inv(pose)[None] @ torch.stack(list(src_poses), 0)
        self.boxes = self._apply_poses(boxes, mm)
        self.size = self.boxes.size(0)
        self.shared_pose = pose

    @staticmethod
    def _apply_poses(src, mm):
        """src [n, 7 | 9], mm [n, 4, 4] -> the boxes moved by mm: centres by the full matrix, headings by its rotation"""
        mm = mm.to(src.dtype).clone()
        center_h = F.pad(src[:, :3], (0, 1), 'constant', 1)
        heading_h = F.pad(_heading_unit_vector(src), (0, 1), 'constant', 1)
        tgt_center = torch.einsum('nij,nj->ni', mm, center_h)[:, :3]
        mm[:, :3, 3] = 0
        tgt_heading = torch.einsum('nij,nj->ni', mm, heading_h)[:, :3]
        tgt_yaw = torch.atan2(tgt_heading[:, 0], tgt_heading[:, 1])
        out = torch.cat([tgt_center, src[:, 3:6], tgt_yaw[:, None]], 1)
        if src.size(1) == 9:
            velo = F.pad(src[:, [7, 8]], (0, 1), 'constant', 0)
            velo = torch.einsum('nij,nj->ni', mm[:, :3, :3], velo)
            out = torch.cat([out, velo[:, :2]], 1)
        return out

    def shared2ego(self, boxes=None, inplace=False):
        """the boxes (default: the tracklet's own) from the shared pose back to every frame's own pose -> [n, 7 | 9]"""
        tgt_pose = torch.stack(list(self.pose_list), 0)
        mm = torch.linalg.inv(tgt_pose) @ self.shared_pose
        src = self.boxes if boxes is None else (boxes.tensor if hasattr(boxes, 'tensor') else boxes)
        out = self._apply_poses(src, mm)
        if inplace:
            assert len(self) == out.size(0)
            self.boxes = out
            return None
        return out

    def centerpoints(self):
        assert self.in_world or self.shared_pose is not None
        return self.boxes[:, :3]

    def to(self, device):
        self.boxes = self.boxes.to(device)
        if getattr(self, 'pose_list', None) is not None:
            self.pose_list = [p.to(device) for p in self.pose_list]
        if getattr(self, 'shared_pose', None) is not None:
            self.shared_pose = self.shared_pose.to(device)
        self.device = self.boxes.device
        return self

    def update_from_prediction(self, boxes, scores, labels, valid_mask, to_numpy=True):
        """lidar_tracklet.py:403-445: the refined boxes, back in every frame's own pose, replace the old ones where the RoI was
        valid; elsewhere the old box (in its own pose) and the old score stay.  One host read (boxes, scores, mask together)."""
        boxes = boxes.tensor if hasattr(boxes, 'tensor') else boxes
        assert len(boxes) == len(scores) == len(labels) == len(valid_mask) == len(self)
        assert (labels == labels[0]).all()
        self.type = int(labels[0])
        if hasattr(self, 'translation_factor'):
            trans_factor = -1 * torch.from_numpy(self.translation_factor).to(self.device)
            boxes = boxes.clone()
            boxes[:, :3] += trans_factor
            self.translate(trans_factor)
        new = self.shared2ego(boxes)
        old = self.shared2ego()
        mask = valid_mask.to(new.device).bool()
        old_scores = self.concated_scores().to(new.device)
        out_boxes = torch.where(mask[:, None], new, old)
        out_scores = torch.where(mask, scores.to(old_scores.dtype), old_scores)
        self.pose_list = None
        self.boxes = out_boxes.cpu() if to_numpy else out_boxes
        self.score_list = out_scores.tolist()

    def merge_not_exist(self, trk):
        """frames ``trk`` has and this tracklet lacks are taken from ``trk`` (lidar_tracklet.py:604-631)"""
        all_ts = sorted(list(set(self.ts_list + trk.ts_list)))
        rows, scores, poses = [], [], []
        with_pose = getattr(self, 'pose_list', None) is not None
        for ts in all_ts:
            src, idx = (self, self.ts2index[ts]) if ts in self.ts2index else (trk, trk.ts2index[ts])
            rows.append(src.boxes[idx:idx + 1].to(self.boxes.device))
            scores.append(src.score_list[idx])
            if with_pose:
                poses.append(src.pose_list[idx])
        self.boxes = torch.cat(rows, 0)
        self.score_list, self.ts_list = scores, all_ts
        if with_pose:
            self.pose_list = poses
        self.freeze()


for _name in REFUSED_METHODS:
    setattr(LiDARTracklet, _name, (lambda n: lambda self, *a, **k: _refuse(n))(_name))


# ---- the fused targets ---------------------------------------------------------------------------------------------------

def _per_class(value, n, what):
    vals = [float(v) for v in value] if isinstance(value, (list, tuple)) else [float(value)] * n
    if len(vals) < n:
        raise RuntimeError(f'tracklet_targets: {what} needs one value per class ({n}), got {len(vals)}')
    return vals[:n]


def _pack(ints, floats, dev):
    """int64 arrays and fp32 arrays -> views of ONE device buffer filled by one pinned host buffer and one copy"""
    n_i, n_f = sum(a.size for a in ints), sum(a.size for a in floats)
    nbytes = 8 * n_i + 4 * n_f
    host = torch.empty(max(nbytes, 8), dtype=torch.uint8)
    if torch.cuda.is_available():
        host = host.pin_memory()
    hi, hf = host[:8 * n_i].view(torch.int64), host[8 * n_i:nbytes].view(torch.float32)
    o = 0
    for a in ints:
        hi[o:o + a.size] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64).reshape(-1))
        o += a.size
    o = 0
    for a in floats:
        hf[o:o + a.size] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1))
        o += a.size
    buf = host.to(dev, non_blocking=True)
    di, df = buf[:8 * n_i].view(torch.int64), buf[8 * n_i:nbytes].view(torch.float32)
    out_i, out_f, o = [], [], 0
    for a in ints:
        out_i.append(di[o:o + a.size])
        o += a.size
    o = 0
    for a in floats:
        out_f.append(df[o:o + a.size].view(a.shape))
        o += a.size
    return out_i, out_f


def _host_boxes(trk):
    b = trk.boxes
    if b.size(0) and b.size(1) != 7:
        b = b[:, :7]
    return b.detach().cpu().numpy().reshape(-1, 7) if not b.is_cuda else None


@torch.no_grad()
def tracklet_targets(tracklets, candidates_list, train_cfg=None, *, device=None, num_classes=None, class_indices=None, **over):
    """_select_one2one_candidates + _assign_and_sample + get_targets of the reference for a batch of tracklets: one launch,
    nothing read back.

    tracklets: LiDARTracklet per batch member (frozen; boxes on the host or on the device); candidates_list: per member the list
    of its ground-truth candidates.  train_cfg (dict or attribute object; keyword arguments override): candidate_thresh (0.5),
    assigner = dict(object_centric, iou_thr), cls_pos_thr / cls_neg_thr (one float or one per class); merge_candidates is
    refused.  class_indices: the class of every tracklet in [0, num_classes) (default: ``trk.type``, the reference's
    ``trk_gt.type`` in the 'mmdet3d' type format).

    -> dict of device tensors, rows of tracklet t at trk_offsets[t] .. in PseudoSampler's order (positives in frame order, then
    negatives in frame order): rois [R, 8] = (t, box), src int32, gt_index int32 (row of ``gts``), labels int64, iou,
    soft_label, reg_mask uint8, targets [R, 7] - the layout roi_loss takes - and frame_inds int64 (bboxes_frame_inds), scores,
    pos_gt_bboxes [R, 7]; in frame order matched int32, overlaps (self_ious), assigned_gt_inds int64 (AssignResult.gt_inds);
    per tracklet chosen int32 (index into the member's candidates, -1 without one) and counts int32 [T, 2]; gts (all candidate
    boxes), and the host lists trk_lens / cand_lens."""
    cfg = dict(over)

    def get(key, default=None):
        if key in cfg:
            return cfg[key]
        return _cfg_get(train_cfg, key, default) if train_cfg is not None else default

    if get('merge_candidates', False):
        raise NotImplementedError('tracklet_targets: merge_candidates is not built (no shipped config sets it)')
    assigner = get('assigner', None) or {}
    object_centric = bool(cfg.get('object_centric', _cfg_get(assigner, 'object_centric', False)))
    iou_thr = float(cfg.get('iou_thr', _cfg_get(assigner, 'iou_thr', 0.5)))
    candidate_thresh = float(get('candidate_thresh', 0.5))
    T = len(tracklets)
    if T != len(candidates_list):
        raise RuntimeError('tracklet_targets: one candidate list per tracklet expected')
    if class_indices is None:
        class_indices = [int(t.type) for t in tracklets]
    if num_classes is None:
        num_classes = max([3] + [c + 1 for c in class_indices])
    if not 1 <= num_classes <= MAX_CLASSES:
        raise RuntimeError(f'tracklet_targets: 1 to {MAX_CLASSES} classes, got {num_classes}')
    if any(not 0 <= c < num_classes for c in class_indices):
        raise RuntimeError(f'tracklet_targets: class indices within [0, {num_classes}) expected, got {class_indices}')
    cpos = _per_class(get('cls_pos_thr', 0.75), num_classes, 'cls_pos_thr')
    cneg = _per_class(get('cls_neg_thr', 0.25), num_classes, 'cls_neg_thr')
    if device is None:
        device = next((t.boxes.device for t in tracklets if t.boxes.is_cuda), None)
        device = device if device is not None else torch.device('cuda', torch.cuda.current_device())
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('sst_amd: tracklet_targets needs a CUDA/HIP device (no CPU path in this library)')

    cands = [c for cl in candidates_list for c in cl]
    for t in list(tracklets) + cands:
        if not getattr(t, 'frozen', False):
            raise RuntimeError('tracklet_targets: tracklets and candidates must be frozen (freeze())')
    trk_lens, cand_lens = [len(t) for t in tracklets], [len(c) for c in cands]
    trk_off = np.concatenate([[0], np.cumsum(trk_lens)]).astype(np.int64)
    cand_off = np.concatenate([[0], np.cumsum(cand_lens)]).astype(np.int64)
    trk_cand_off = np.concatenate([[0], np.cumsum([len(cl) for cl in candidates_list])]).astype(np.int64)
    R, G, C = int(trk_off[-1]), int(cand_off[-1]), len(cands)
    ts = np.asarray([x for t in tracklets for x in t.ts_list], np.int64).reshape(-1)
    cts = np.asarray([x for c in cands for x in c.ts_list], np.int64).reshape(-1)
    scores = np.asarray([x for t in tracklets for x in t.score_list], np.float32).reshape(-1)
    ints = [ts, trk_off, cts, cand_off, trk_cand_off, np.asarray(class_indices, np.int64)]
    floats = [scores]
    host_b = [_host_boxes(t) for t in tracklets]
    host_c = [_host_boxes(c) for c in cands]
    b_on_host, c_on_host = all(b is not None for b in host_b), all(b is not None for b in host_c)
    if b_on_host:
        floats.append(np.concatenate(host_b + [np.zeros((0, 7), np.float32)], 0))
    if c_on_host:
        floats.append(np.concatenate(host_c + [np.zeros((0, 7), np.float32)], 0))
    (d_ts, d_trk_off, d_cts, d_cand_off, d_trk_cand_off, d_cls), d_floats = _pack(ints, floats, dev)
    d_scores = d_floats[0]
    rest = list(d_floats[1:])
    boxes = rest.pop(0) if b_on_host else torch.cat([t.boxes[:, :7].to(dev) for t in tracklets], 0).float().contiguous()
    if c_on_host:
        gts = rest.pop(0)
    elif cands:
        gts = torch.cat([c.boxes[:, :7].to(dev) for c in cands], 0).float().contiguous()
    else:
        gts = torch.zeros((0, 7), dtype=torch.float32, device=dev)

    def new(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=dev)

    out = dict(rois=new((R, 8), torch.float32), src=new(R, torch.int32), gt_index=new(R, torch.int32), labels=new(R, torch.long),
               iou=new(R, torch.float32), soft_label=new(R, torch.float32), reg_mask=new(R, torch.uint8),
               targets=new((R, 7), torch.float32), frame_inds=new(R, torch.long), scores=new(R, torch.float32),
               pos_gt_bboxes=new((R, 7), torch.float32), matched=new(R, torch.int32), overlaps=new(R, torch.float32),
               assigned_gt_inds=new(R, torch.long), chosen=new(T, torch.int32), counts=new((T, 2), torch.int32))
    a = _lib.TrackletTargetsArgs()
    a.boxes, a.ts, a.scores, a.trk_offsets = boxes.data_ptr(), d_ts.data_ptr(), d_scores.data_ptr(), d_trk_off.data_ptr()
    a.cand_boxes, a.cand_ts, a.cand_offsets = gts.data_ptr(), d_cts.data_ptr(), d_cand_off.data_ptr()
    a.trk_cand_offsets, a.trk_class = d_trk_cand_off.data_ptr(), d_cls.data_ptr()
    a.iou_out, a.scores_out = out['iou'].data_ptr(), out['scores'].data_ptr()
    for k in ('chosen', 'counts', 'matched', 'overlaps', 'assigned_gt_inds', 'rois', 'src', 'frame_inds', 'gt_index', 'labels',
              'soft_label', 'reg_mask', 'targets', 'pos_gt_bboxes'):
        setattr(a, k, out[k].data_ptr())
    a.n_rows, a.n_cand_rows, a.n_cands, a.n_tracklets = R, G, C, T
    a.num_classes, a.object_centric = int(num_classes), 1 if object_centric else 0
    a.candidate_thresh, a.iou_thr = candidate_thresh, iou_thr
    for i in range(num_classes):
        a.cls_pos_thr[i], a.cls_neg_thr[i] = cpos[i], cneg[i]
    if T:
        _lib.check(_lib.load().sst_tracklet_targets_f32(ctypes.byref(a), _lib.stream_ptr()), 'sst_tracklet_targets_f32')
    # chosen: from the index into all candidates to the index within the member's own list
    out['chosen'] = torch.where(out['chosen'] >= 0, out['chosen'] - d_trk_cand_off[:-1].to(torch.int32), out['chosen'])
    out.update(boxes=boxes, gts=gts, trk_offsets=d_trk_off, trk_lens=trk_lens, cand_lens=cand_lens,
               cands_per_tracklet=[len(cl) for cl in candidates_list])
    return out


class AssignResult(object):
    """mmdet's AssignResult as TrackletAssigner fills it"""

    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels


class TrackletAssigner(object):
    """core/bbox/assigners/tracklet_assigner.py: every box of a predicted tracklet is assigned the ground-truth box of the same
    timestamp (with object_centric only where their IoU exceeds iou_thr) - a one-tracklet call of the targets kernel."""

    def __init__(self, object_centric=False, iou_thr=0.5):
        self.object_centric = object_centric
        self.iou_thr = iou_thr

    def assign(self, trk_pd, trk_gt):
        num_classes = max(3, int(trk_gt.type) + 1, int(trk_pd.type) + 1)
        res = tracklet_targets([trk_pd], [[trk_gt]], None, object_centric=self.object_centric, iou_thr=self.iou_thr,
                               class_indices=[max(int(trk_gt.type), 0)], num_classes=num_classes)
        gt_inds = res['assigned_gt_inds']
        labels = torch.where(gt_inds > 0, torch.full_like(gt_inds, int(trk_gt.type)), torch.full_like(gt_inds, -1))
        out = AssignResult(len(trk_gt), gt_inds, res['overlaps'], labels=labels)
        out.scores = res['scores'].new_empty(len(trk_pd))
        out.scores[res['frame_inds']] = res['scores']
        out.targets = res
        return out


# ---- the input rows of the box head ------------------------------------------------------------------------------------------

class _TrackletRows(torch.autograd.Function):

    @staticmethod
    def forward(ctx, pts_feats, pts_xyz, pts_frame_inds, pts_inds, roi_inds, roi_frame_inds, roi_scores, combined, with_roi_scores):
        m, n, f = pts_inds.numel(), pts_feats.size(0), pts_feats.size(1)
        w = f + int(combined) + int(with_roi_scores)
        out = torch.empty((m, w), dtype=torch.float32, device=pts_feats.device)
        xyz_out = torch.empty((m, pts_xyz.size(1)), dtype=torch.float32, device=pts_feats.device)
        a = _lib.TrackletRowsArgs()
        a.feats, a.xyz, a.pts_inds, a.out, a.xyz_out = (pts_feats.data_ptr(), pts_xyz.data_ptr(), pts_inds.data_ptr(), out.data_ptr(),
                                                        xyz_out.data_ptr())
        if combined or with_roi_scores:
            a.roi_inds = roi_inds.data_ptr()
        if combined:
            a.pts_frame_inds, a.roi_frame_inds = pts_frame_inds.data_ptr(), roi_frame_inds.data_ptr()
        if with_roi_scores:
            a.roi_scores = roi_scores.data_ptr()
        n_rois = roi_frame_inds.numel() if combined else (roi_scores.numel() if with_roi_scores else 0)
        a.m, a.n_points, a.n_rois, a.ld_feats, a.ld_xyz = m, n, n_rois, pts_feats.stride(0), pts_xyz.stride(0)
        a.feat_cols, a.xyz_cols, a.combined, a.with_roi_scores = f, pts_xyz.size(1), int(combined), int(with_roi_scores)
        _lib.check(_lib.load().sst_tracklet_rows_fwd_f32(ctypes.byref(a), _lib.stream_ptr()), 'sst_tracklet_rows_fwd_f32')
        ctx.save_for_backward(pts_inds)
        ctx.shape = (m, n, f, w)
        ctx.mark_non_differentiable(xyz_out)
        return out, xyz_out

    @staticmethod
    def backward(ctx, g_out, _g_xyz):
        (pts_inds,) = ctx.saved_tensors
        m, n, f, w = ctx.shape
        dev = pts_inds.device
        g_out = g_out.contiguous()
        # key = point * m + row: sorted, the rows of a point are one run in ascending row order (distinct keys: any sort will do)
        lib = _lib.load()
        keys = torch.empty(m, dtype=torch.long, device=dev)
        _lib.check(lib.sst_tracklet_rows_keys_i64(_lib.ptr(pts_inds), m, n, _lib.ptr(keys), _lib.stream_ptr()), 'sst_tracklet_rows_keys_i64')
        keys = torch.sort(keys)[0]
        d_feats = torch.empty((n, f), dtype=torch.float32, device=dev)
        _lib.check(lib.sst_tracklet_rows_bwd_f32(_lib.ptr(g_out), m, w, f, _lib.ptr(keys), n, _lib.ptr(d_feats), _lib.stream_ptr()),
                   'sst_tracklet_rows_bwd_f32')
        return (d_feats,) + (None,) * 8


def tracklet_rows(pts_feats, pts_xyz, pts_frame_inds, ext_pts_inds, ext_pts_roi_inds, roi_frame_inds=None, roi_scores=None, *,
                  combined=True, with_roi_scores=False):
    """the input rows of the box head (tracklet_roi_head.py:247-258) -> (new_pts_feats [M, F (+ 1) (+ 1)], new_pts_xyz [M, 3 ..]):
    pts_feats[ext_pts_inds] | is_cur_frame (combined) | roi_scores[ext_pts_roi_inds] (with_roi_scores), and pts_xyz[ext_pts_inds],
    in one launch; the gradient of pts_feats in one launch with a fixed order of the additions.  Index -1 (the pool's fake row)
    reads the last row, as the reference's indexing does."""
    _lib.require_cuda(pts_feats, ext_pts_inds, ext_pts_roi_inds)
    if pts_feats.dtype != torch.float32 or pts_xyz.dtype != torch.float32:
        raise RuntimeError('tracklet_rows: float32 features and points expected')
    if pts_feats.dim() != 2 or pts_xyz.dim() != 2 or pts_xyz.size(0) != pts_feats.size(0) or pts_xyz.size(1) > 16:
        raise RuntimeError(f'tracklet_rows: pts_feats [N, F] and pts_xyz [N, <= 16] expected, got {tuple(pts_feats.shape)}, {tuple(pts_xyz.shape)}')
    if pts_feats.stride(1) != 1 or pts_xyz.stride(1) != 1:
        pts_feats, pts_xyz = pts_feats.contiguous(), pts_xyz.contiguous()
    if ext_pts_inds.dtype != torch.long or ext_pts_roi_inds.dtype != torch.long or ext_pts_inds.shape != ext_pts_roi_inds.shape:
        raise RuntimeError('tracklet_rows: int64 ext_pts_inds and ext_pts_roi_inds of one shape expected')
    if pts_feats.size(0) == 0:
        raise RuntimeError('tracklet_rows: no point to read')
    if combined:
        if roi_frame_inds is None or pts_frame_inds is None:
            raise RuntimeError('tracklet_rows: the combined form needs pts_frame_inds and roi_frame_inds')
        pts_frame_inds, roi_frame_inds = pts_frame_inds.to(torch.long).contiguous(), roi_frame_inds.to(torch.long).contiguous()
        _lib.require_cuda(pts_frame_inds, roi_frame_inds)
        if pts_frame_inds.numel() != pts_feats.size(0):
            raise RuntimeError('tracklet_rows: one frame index per point expected')
    if with_roi_scores:
        if roi_scores is None:
            raise RuntimeError('tracklet_rows: with_roi_scores needs roi_scores')
        roi_scores = roi_scores.detach().to(torch.float32).contiguous()
        _lib.require_cuda(roi_scores)
        if combined and roi_scores.numel() != roi_frame_inds.numel():
            raise RuntimeError('tracklet_rows: one score and one frame index per RoI expected')
    return _TrackletRows.apply(pts_feats, pts_xyz, pts_frame_inds, ext_pts_inds.contiguous(), ext_pts_roi_inds.contiguous(),
                               roi_frame_inds, roi_scores, bool(combined), bool(with_roi_scores))
