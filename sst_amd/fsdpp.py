"""TwoStageFSDPP (mmdet3d/models/detectors/two_stage_fsdpp.py of the reference): FSD with the incremental point stage in front
of its segmentor.  Everything behind the stage is FSD's (``sst_amd.detectors.FSD``); the stage is ``sst_amd.incremental`` over
csrc/incremental.hip.  The stage owns no parameter: the ``state_dict`` keys equal FSD's.

Training (``forward_train``): generate_points for the whole batch, then FSD.forward_train.  Sequential testing (``simple_test``
with ``test_cfg.reuse_test``): the reference's ``reuse_simple_test`` - per segment queues of the previous clouds, poses, results
and crops, every cloud moved into the current frame by one transform launch per 8 clouds, matrices formed on the host in
float64.

Refused by name (NotImplementedError): roi_head type IncrementalROIHead; incremental_cfg n_fps, voxel_pooling_size,
crop_painting, virtual_seed_points_cfg, noise_cfg, pre_nms_thr, elegant_max_age; aug_test.  The dataset, LoadPreviousFramesWaymo
and the hook classes are not part of this library.
"""
import copy

import numpy as np
import torch
import torch.nn.functional as F

from . import incremental as I
from ._head_common import cfg_get as _get
from .detectors import DETECTORS, FSD


def _index_seed(seed, mask):
    """{k: v[mask]} of filter_seed_by_score for numpy arrays, tensors and box objects"""
    out = {}
    for k, v in seed.items():
        if isinstance(v, np.ndarray):
            out[k] = v[mask]
        else:
            m = torch.from_numpy(np.asarray(mask))
            t = v.tensor if hasattr(v, 'tensor') else v
            out[k] = v[m.to(t.device)]
    return out


@DETECTORS.register_module()
class TwoStageFSDPP(FSD):
    """two_stage_fsdpp.py:36-979"""

    def __init__(self, backbone, segmentor, roi_head=None, incremental_cfg=None, **kw):
        if incremental_cfg is None:
            raise RuntimeError('TwoStageFSDPP: incremental_cfg is required')
        rcnn_type = _get(roi_head, 'type', None)
        if rcnn_type == 'IncrementalROIHead':
            raise NotImplementedError('TwoStageFSDPP: roi_head type IncrementalROIHead is not built (no shipped config uses it)')
        if rcnn_type != 'GroupCorrectionHead':
            raise NotImplementedError(f'TwoStageFSDPP: roi_head type {rcnn_type} (GroupCorrectionHead expected)')
        I.refuse_cfg(incremental_cfg, 'TwoStageFSDPP')
        super().__init__(backbone, segmentor, roi_head=roi_head, **kw)
        self.incremental_cfg = incremental_cfg
        self.max_pre_frames = _get(incremental_cfg, 'num_previous_frames', 4)
        self.rcnn_type = rcnn_type
        self.iters = 0
        self.last_segind = 'None'
        self._reset_sequence()

    def _reset_sequence(self):
        self.previous_pc = []
        self.previous_delta_pc = []
        self.previous_sample_idx = []
        self.previous_pose = []          # host float64 [4, 4] of the fp32 pose
        self.previous_seed_info = []
        self.previous_cropped_pc = []
        self.frame_counter = 0

    # ---- seeds -----------------------------------------------------------------------------------------------------------

    def filter_seed_by_score(self, seed_all_frames):
        new_list = []
        for seed in seed_all_frames:
            scores = seed['scores']
            if len(scores) == 0:
                new_list.append(seed)
                continue
            s = scores.detach().cpu().numpy() if torch.is_tensor(scores) else np.asarray(scores)
            new_list.append(_index_seed(seed, s > self.incremental_cfg['pre_score_thr']))
        return new_list

    def preprocess_seed(self, seed_list, device=None):
        """:824-846: the score filter and the cut to num_previous_frames"""
        score_thr = _get(self.incremental_cfg, 'pre_score_thr', 0)
        if score_thr > 0:
            if not self.training:
                assert score_thr == self.test_cfg['rcnn']['score_thr'], 'training-testing consistency'
            seed_list = [self.filter_seed_by_score(s) for s in seed_list]
        I.refuse_cfg(self.incremental_cfg, 'TwoStageFSDPP')
        return [s[:self.max_pre_frames] for s in seed_list]

    def modify_previous_boxes(self, seed_info, device):
        """:763-798 -> dict(gt_bboxes_3d = the enlarged [n, 7] device tensor, origin_bboxes, gt_labels_3d, scores)"""
        boxes = I._box_tensor(seed_info['gt_bboxes_3d'])
        if len(boxes) == 0:
            return seed_info
        boxes = torch.as_tensor(boxes).to(device)
        labels, scores = seed_info['gt_labels_3d'], seed_info['scores']
        if isinstance(scores, np.ndarray):
            labels = torch.from_numpy(labels).to(device).float()
            scores = torch.from_numpy(scores).to(device).float()
        else:
            labels, scores = labels.clone(), scores.clone()
        return dict(origin_bboxes=boxes.clone(), gt_labels_3d=labels, scores=scores,
                    gt_bboxes_3d=I.enlarge_boxes(boxes, labels, self.incremental_cfg, self.training))

    def crop_and_process_points(self, points, seed_info):
        """:637-678 over the stage's kernels (one cloud, one set of boxes); the rows come in ascending input index"""
        cfg = self.incremental_cfg
        max_n = int(_get(cfg, 'max_crop_points', 0) or 0)
        keys = None
        if max_n > 0 and _get(cfg, 'crop_shuffle', False) and len(points) > 0:
            keys = torch.randint(0, 2 ** 32, (len(points),), dtype=torch.int64, device=points.device)
        return I.seed_crop(points, seed_info['gt_bboxes_3d'], max_n, keys)

    def result2seed(self, results, device):
        res = results[0]
        if isinstance(res, dict):
            boxes, scores, labels = res['boxes_3d'], res['scores_3d'], res['labels_3d']
        else:
            boxes, scores, labels = res
        return dict(gt_bboxes_3d=I._box_tensor(boxes).to(device), gt_labels_3d=labels.to(device), scores=scores.float().to(device))

    # ---- training ----------------------------------------------------------------------------------------------------------

    def generate_points(self, points, pts_frame_inds, seed_info, keys=None):
        """:460-503 for the whole batch in one pass of the stage"""
        return I.generate_points(points, pts_frame_inds, seed_info, self.incremental_cfg, self.training, keys=keys)

    def forward_train(self, points, pts_frame_inds, img_metas, gt_bboxes_3d, gt_labels_3d, seed_info=None, gt_bboxes_ignore=None):
        """:92-185: generate_points, then FSD.forward_train (point drop, RPN step, RoI input, RoI losses).  num_input_points counts
        the points that survive the drop, as the reference's does."""
        self._require_heads('forward_train')
        seed_info = self.preprocess_seed(seed_info)
        new_points, num_delta = self.generate_points(points, pts_frame_inds, seed_info)
        ratio = _get(self.train_cfg, 'point_drop_ratio', 0)
        kept = [int(len(p) * (1 - ratio)) if ratio > 0 else len(p) for p in new_points]
        self.print_info['num_input_points'] = new_points[0].new_zeros(1) + sum(kept) / len(new_points)
        self.print_info['num_delta_points'] = new_points[0].new_zeros(1) + sum(num_delta) / len(new_points)
        return FSD.forward_train(self, new_points, img_metas, gt_bboxes_3d, gt_labels_3d, gt_bboxes_ignore=gt_bboxes_ignore)

    # ---- testing -----------------------------------------------------------------------------------------------------------

    def aug_test(self, *args, **kwargs):
        raise NotImplementedError('TwoStageFSDPP.aug_test is not built')

    def simple_test(self, points, img_metas, imgs=None, pts_frame_inds=None, seed_info=None, pose=None, rescale=False,
                    gt_bboxes_3d=None, gt_labels_3d=None):
        """:259-278"""
        assert len(seed_info) == 1
        seed_info = self.preprocess_seed(seed_info[0])
        if _get(self.test_cfg, 'reuse_test', False):
            assert self.test_cfg['sequential']
            return self.reuse_simple_test(points, img_metas, imgs, pts_frame_inds, seed_info, pose, rescale, gt_bboxes_3d,
                                          gt_labels_3d)
        raise NotImplementedError('Need to change the data config, adding LoadPreviousFramesWaymo')

    def input_agnostic_simple_test(self, points, img_metas, seed_info=None, gt_bboxes_3d=None, gt_labels_3d=None):
        """:280-351 with GroupCorrectionHead = FSD.simple_test"""
        return FSD.simple_test(self, points, img_metas, gt_bboxes_3d=gt_bboxes_3d, gt_labels_3d=gt_labels_3d)

    def reuse_simple_test(self, points, img_metas, imgs=None, pts_frame_inds=None, seed_info=None, pose=None, rescale=False,
                          gt_bboxes_3d=None, gt_labels_3d=None):
        """:353-402, the sequential path"""
        assert len(seed_info) == 1
        seed_info = seed_info[0]
        assert pts_frame_inds is None
        cur_points = points
        device = cur_points[0].device
        sample_idx = img_metas[0]['sample_idx']
        segment_idx = f'{sample_idx:07d}'[1:4]
        if self.last_segind != segment_idx:
            self._reset_sequence()
        p0 = pose[0]
        curr_pose = I._host64(p0.squeeze().float() if torch.is_tensor(p0) else np.asarray(p0, np.float32).squeeze())
        seed_info = self.get_seed_info(img_metas, seed_info, curr_pose, device)
        merged_pc = self.filter_and_merge_pc(cur_points, segment_idx, curr_pose, seed_info)
        results = self.input_agnostic_simple_test([merged_pc, ], img_metas, seed_info, gt_bboxes_3d, gt_labels_3d)
        cur_seed = self.result2seed(results, device)
        self.previous_seed_info.append(cur_seed)
        self.frame_counter += 1
        cur_modified_seed = self.modify_previous_boxes(cur_seed, device)
        self.previous_cropped_pc.append(self.crop_and_process_points(cur_points[0], cur_modified_seed))
        if len(self.previous_pc) > self.max_pre_frames:
            self.previous_pc.pop(0)
            self.previous_sample_idx.pop(0)
            self.previous_pose.pop(0)
            self.previous_seed_info.pop(0)
            self.previous_cropped_pc.pop(0)
        self.last_segind = segment_idx
        return results

    def get_seed_info(self, img_metas, offline_seed_info, cur_pose, device):
        """:950-979.  As in the reference, the stored boxes of a previous result are moved by inv(cur_pose) @ (their frame's
        pose) at EVERY later frame, in place."""
        if not _get(self.test_cfg, 'reuse_results', False):
            return offline_seed_info
        assert self.test_cfg['sequential']
        assert len(self.previous_seed_info) == len(self.previous_pose)
        assert len(self.previous_seed_info) <= self.max_pre_frames
        cur_pose_inv = np.linalg.inv(cur_pose)
        for seed, pre_pose in zip(self.previous_seed_info, self.previous_pose):
            seed['gt_bboxes_3d'] = I.box_frame_transform_gpu(seed['gt_bboxes_3d'], pre_pose, None, cur_pose_inv=cur_pose_inv)
        calib_interval = _get(self.test_cfg, 'calib_interval', -1)
        if calib_interval != -1 and (self.frame_counter + 1) % calib_interval == 0 and len(self.previous_seed_info) > 0:
            last_seed = copy.deepcopy(offline_seed_info[0])
            last_seed['gt_bboxes_3d'] = I._box_tensor(last_seed['gt_bboxes_3d']).to(device)
            last_seed['gt_labels_3d'] = torch.from_numpy(np.asarray(last_seed['gt_labels_3d'])).to(device).float()
            last_seed['scores'] = torch.from_numpy(np.asarray(last_seed['scores'])).to(device).float()
            self.previous_seed_info[-1] = last_seed
        if len(self.previous_seed_info) < self.max_pre_frames:
            return offline_seed_info
        return [self.previous_seed_info[-i - 1] for i in range(len(self.previous_seed_info))]

    def _into_current(self, clouds, poses, cur_pose):
        """every cloud [n, C] of a queue in the current frame: one launch per 8 clouds"""
        inv = np.linalg.inv(cur_pose)
        return I.transform_clouds(clouds, [I.frame_matrix(p, None, cur_pose_inv=inv) for p in poses])

    def filter_and_merge_pc(self, points, sample_idx, curr_pose, seed_info):
        """:404-433"""
        assert len(self.previous_pc) <= self.max_pre_frames
        points = points[0]
        previous_pc_incurr = self._into_current(self.previous_pc, self.previous_pose, curr_pose)
        out_points_list, _ = self.generate_points_list(points, previous_pc_incurr, seed_info, curr_pose)
        self.previous_pc.append(points)
        self.previous_pose.append(curr_pose)
        self.previous_sample_idx.append(sample_idx)
        assert len(set(self.previous_sample_idx)) == 1
        return out_points_list[0]

    def generate_points_list(self, cur_points, pre_points_list, seed_info, cur_pose):
        """:528-565"""
        assert not self.training, 'only used in single-sample testing'
        cfg = self.incremental_cfg
        if len(seed_info) > len(pre_points_list):
            pre_points_list.append(cur_points)
            assert len(seed_info) == len(pre_points_list), f'{len(seed_info)} {len(pre_points_list)}'
        old_points = self.get_old_points_list_v2(cur_points, seed_info, cur_pose)
        if _get(cfg, 'disable_incremental', False):
            return [old_points, ], [0, ]
        num_base_frame = _get(cfg, 'num_base_frame', self.max_pre_frames)
        delta_points = self.get_delta_points_list(cur_points, pre_points_list[-num_base_frame:])
        num_delta_points = len(delta_points)
        delta_points = F.pad(delta_points, (0, 1), 'constant', 0)
        if _get(cfg, 'max_age', 0) > 0:
            last = self.get_delta_points_list(pre_points_list[-1], pre_points_list[-num_base_frame:-1])
            delta_points = torch.cat([delta_points, F.pad(last, (0, 1), 'constant', -0.1)], 0)
        return [torch.cat([old_points, delta_points], dim=0), ], [num_delta_points, ]

    def get_delta_points_list(self, cur_points, pre_points_list):
        """:747-755"""
        cfg = self.incremental_cfg
        if len(pre_points_list) > 0:
            return I.find_delta_points_by_voxelization_list_v3(pre_points_list, cur_points, cfg['voxel_size'], cfg['point_cloud_range'])
        return cur_points.new_zeros((0, cur_points.size(1)))

    def get_delta_points(self, cur_points, pre_points):
        """:738-745"""
        cfg = self.incremental_cfg
        if len(pre_points) > 0:
            return I.find_delta_points_by_voxelization(pre_points, cur_points, cfg['voxel_size'], cfg['point_cloud_range'])
        return cur_points.new_zeros((0, cur_points.size(1)))

    def get_old_points_list_v2(self, cur_points, frames_seed_info, cur_pose):
        """:696-736"""
        device = cur_points.device
        assert len(self.previous_cropped_pc) == len(self.previous_pose)
        pre_crop_pc = list(self._into_current(self.previous_cropped_pc, self.previous_pose, cur_pose))
        if len(frames_seed_info) > len(pre_crop_pc):
            # the warm-up stage of a sequence: the current frame is cropped by the newest seed
            padding_seed = self.modify_previous_boxes(frames_seed_info[0], device)
            pre_crop_pc.append(self.crop_and_process_points(cur_points, padding_seed))
            assert len(frames_seed_info) == len(pre_crop_pc)
        if 'crop_frames' in self.incremental_cfg:
            crop_frames = min(self.incremental_cfg['crop_frames'], len(pre_crop_pc))
            pre_crop_pc = pre_crop_pc[-crop_frames:]
        out_pc_list = [F.pad(pc, (0, 1), 'constant', float(i - len(pre_crop_pc)) / 10) for i, pc in enumerate(pre_crop_pc)]
        out_points = torch.cat(out_pc_list, dim=0)
        if len(out_points) < 500:
            # too few points may lead to an error in the sparse convolutions
            out_points = torch.cat([F.pad(cur_points[:500, :], (0, 1), 'constant', 0), out_points], 0)
        return out_points
