"""TwoStageFSDPP on the GPU: configs/fsdpp/fsdpp_waymoD1_1x_7f_6base.py (tests/golden/configs/fsdpp) with the range cut to
51.2 m x 51.2 m and sparse_shape to [32, 256, 256].  forward_train returns finite losses with the segmentor's, the cluster head's
and the RoI head's keys and the two counters, equals FSD.forward_train fed with generate_points' output under the same seeds bit
for bit, and sends gradients into the segmentor.  The sequential simple_test over five frames of one segment feeds the network
the cloud the restatement (tests/incremental_ref.py) composes step by step from its own queues, returns what FSD.simple_test
returns for that cloud, keeps queues of the reference's lengths and resets them on a new segment id."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import incremental_ref as R
from test_configs_build import FIXTURES

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RANGE = [-25.6, -25.6, -2, 25.6, 25.6, 4]
SEG_KEYS = {'loss_sem_seg', 'loss_vote', 'recall_Car', 'recall_Ped', 'recall_Cyc'}
RPN_KEYS = {'num_clusters', 'num_fg_points'} | {f'{k}.task{t}' for k in ('loss_cls', 'loss_center', 'loss_size', 'loss_rot')
                                                for t in range(3)}


def small_model(**incr):
    model = eval(open(os.path.join(FIXTURES, 'fsdpp', 'fsdpp_waymoD1_1x_7f_6base.model.py')).read())
    seg = model['segmentor']
    seg['voxel_layer']['point_cloud_range'] = seg['voxel_encoder']['point_cloud_range'] = seg['decode_neck']['point_cloud_range'] = RANGE
    seg['backbone']['sparse_shape'] = [32, 256, 256]
    model['cluster_assigner']['point_cloud_range'] = RANGE
    model['incremental_cfg']['point_cloud_range'] = RANGE
    model['incremental_cfg'].update(incr)
    return model


def build(**incr):
    import sst_amd
    torch.manual_seed(0)
    det = sst_amd.build_detector(small_model(**incr)).attach_heads().to(DEV)
    det.runtime_info = dict(enable_detection=True)
    return det


def frame_cloud(seed, shift):
    """one frame of a scene: the same objects, moved by ``shift`` metres along x, re-sampled"""
    import bench_workloads as BW
    c = BW.chain_cloud(1500, seed, half_extent=12.0)
    keep = torch.randperm(1500, generator=torch.Generator().manual_seed(seed * 7 + int(shift * 10)))[:1300]
    c = c[keep]
    c[:, 0] += shift
    return c


def seed_frames(cloud, n_frames, seed):
    g = np.random.default_rng(seed)
    frames = []
    for i in range(n_frames):
        centre = cloud[g.integers(len(cloud) // 2, len(cloud), 4), :3].cpu().numpy()
        b = np.zeros((4, 7), np.float32)
        b[:, :2], b[:, 2] = centre[:, :2], centre[:, 2] - 0.8
        b[:, 3:6], b[:, 6] = [1.6, 3.0, 1.6], g.uniform(-3, 3, 4)
        frames.append(dict(gt_bboxes_3d=b, gt_labels_3d=g.integers(0, 3, 4), scores=g.uniform(0.2, 1, 4).astype(np.float32)))
    return frames


def calibrate(det, clouds):
    """scale and bias the segmentation head's last layer so that every class selects between 5 % and 60 % of the points"""
    import fsd_sample_ref as S
    head = det.segmentor.segmentation_head
    thr = torch.tensor(S.thresholds32(det.cfg['score_thresh']), device=DEV)
    with torch.no_grad():
        spread = 2.0 / det.segmentor([c.clone() for c in clouds])['seg_logits'].std(0)
        head.conv_seg.weight.mul_(spread[:, None])
        head.conv_seg.bias.mul_(spread)
        logits = det.segmentor([c.clone() for c in clouds])['seg_logits']
        head.conv_seg.bias.add_(torch.log(thr / (1 - thr)) - torch.quantile(logits, 0.7, dim=0))
        share = (det.segmentor([c.clone() for c in clouds])['seg_logits'].sigmoid() > thr[None]).float().mean(0)
    assert bool(((share > 0.05) & (share < 0.6)).all()), share


def train_batch():
    pts, finds, seeds, boxes, labels = [], [], [], [], []
    for s in range(2):
        frames = [frame_cloud(5 + s, 0.4 * k).to(DEV) for k in range(4)]
        pts.append(torch.cat(frames, 0))
        finds.append(torch.arange(4).repeat_interleave(1300).neg().long().to(DEV))
        seeds.append(seed_frames(frames[0], 3, 20 + s))
        centre = frames[0][[1299, 1000, 700], :3].cpu()
        b = torch.zeros(3, 7)
        b[:, :2], b[:, 2] = centre[:, :2], centre[:, 2] - 0.8
        b[:, 3:6], b[:, 6] = torch.tensor([1.6, 3.0, 1.6]), torch.tensor([0.3, -1.0, 2.0]) + s
        boxes.append(b.to(DEV))
        labels.append(torch.tensor([0, 1, 2], device=DEV))
    return pts, finds, seeds, boxes, labels


def _total(losses):
    return sum(v.sum() if torch.is_tensor(v) else sum(x.sum() for x in v)
               for k, v in losses.items() if (torch.is_tensor(v) and v.requires_grad) or isinstance(v, (list, tuple)))


def test_forward_train():
    import sst_amd
    det = build(num_previous_frames=3, crop_frames=3, num_base_frame=2).train()
    pts, finds, seeds, boxes, labels = train_batch()
    metas = [{} for _ in pts]
    with torch.no_grad():
        clouds, _ = det.generate_points(pts, finds, det.preprocess_seed(seeds))
    calibrate(det, clouds)
    torch.manual_seed(1)
    losses = det.forward_train([p.clone() for p in pts], finds, metas, boxes, labels, seed_info=seeds)
    assert SEG_KEYS | RPN_KEYS | {'loss_rcnn_cls', 'loss_rcnn_bbox', 'num_input_points', 'num_delta_points'} <= set(losses)
    for k, v in losses.items():
        for x in (v if isinstance(v, (list, tuple)) else [v]):
            assert bool(torch.isfinite(x).all()), k
    _total(losses).backward()
    grads = [p.grad for p in det.segmentor.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads) and max(float(g.abs().max()) for g in grads) > 0
    det.zero_grad(set_to_none=True)
    # the same step composed by hand: the stage, then FSD's step, under the same seeds
    torch.manual_seed(1)
    new_points, num_delta = det.generate_points([p.clone() for p in pts], finds, det.preprocess_seed(seeds))
    want = sst_amd.FSD.forward_train(det, new_points, metas, boxes, labels)
    assert set(want) == set(losses)
    for k in want:
        a, b = losses[k], want[k]
        a, b = (torch.stack(list(a)), torch.stack(list(b))) if isinstance(b, (list, tuple)) else (a, b)
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), k
    ratio = det.train_cfg['point_drop_ratio']
    assert float(losses['num_input_points']) == sum(int(len(p) * (1 - ratio)) for p in new_points) / 2
    assert float(losses['num_delta_points']) == sum(num_delta) / 2 and min(num_delta) > 0
    assert all(p.size(1) == 6 for p in new_points)


def _pose(t):
    yaw = 0.02 * t
    m = np.eye(4, dtype=np.float64)
    m[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    m[:3, 3] = [1000.0 + 0.4 * t, -2000.0 + 0.1 * t, 30.0]
    return torch.from_numpy(m.astype(np.float32))


def _v3(pre_list, cur, cfg):
    if len(pre_list) == 0:
        return cur.new_zeros((0, cur.size(1)))
    return R.find_delta_points_by_voxelization_list_v3(pre_list, cur, cfg['voxel_size'], cfg['point_cloud_range'])


def test_sequential_simple_test():
    import sst_amd
    from sst_amd import incremental as I
    max_pre, cap = 2, 16
    det = build(num_previous_frames=max_pre, crop_frames=max_pre, num_base_frame=max_pre, crop_shuffle=False, max_crop_points=cap).eval()
    cfg = det.incremental_cfg
    clouds = [frame_cloud(9, 0.4 * t).to(DEV) for t in range(6)]
    calibrate(det, [F.pad(c, (0, 1)) for c in clouds[:2]])
    fed = []
    plain = det.input_agnostic_simple_test

    def recording(points, *args, **kwargs):
        fed.append(points[0].clone())
        return plain(points, *args, **kwargs)
    det.input_agnostic_simple_test = recording
    prev_pc, prev_pose, prev_crop, prev_seed = [], [], [], []
    lengths = []
    with torch.no_grad():
        for t in range(5):
            cur, pose = clouds[t], _pose(t)
            offline = seed_frames(cur, min(t + 1, max_pre), 30 + t)
            results = det.simple_test([cur.clone()], [dict(sample_idx=1003000 + t)], seed_info=[[copy.deepcopy(offline)]], pose=[pose[None]])
            # ---- the same frame composed from the restatement's own queues -------------------------------------------
            for seed, pk in zip(prev_seed, prev_pose):
                seed['boxes'] = I.box_frame_transform_gpu(seed['boxes'], pk, pose)
            if len(prev_seed) < max_pre:
                seed_boxes = [torch.from_numpy(f['gt_bboxes_3d']).to(DEV) for f in offline]
            else:
                seed_boxes = [s['boxes'] for s in reversed(prev_seed)]
            pre_in_cur = [R.frame_transform(pc, I.frame_matrix(pk, pose)) for pc, pk in zip(prev_pc, prev_pose)]
            crops = [R.frame_transform(pc, I.frame_matrix(pk, pose)) for pc, pk in zip(prev_crop, prev_pose)]
            if len(seed_boxes) > len(pre_in_cur):
                pre_in_cur.append(cur)
            if len(seed_boxes) > len(crops):
                b = R.enlarged(seed_boxes[0], cfg['extra_width']) if len(seed_boxes[0]) else seed_boxes[0]
                crops.append(cur[R.crop_indices(cur, b, cap)])
            crops = crops[-min(cfg['crop_frames'], len(crops)):]
            old = torch.cat([F.pad(pc, (0, 1), 'constant', float(i - len(crops)) / 10) for i, pc in enumerate(crops)], 0)
            if len(old) < 500:
                old = torch.cat([F.pad(cur[:500], (0, 1), 'constant', 0), old], 0)
            delta = F.pad(_v3(pre_in_cur[-max_pre:], cur, cfg), (0, 1), 'constant', 0)
            last = F.pad(_v3(pre_in_cur[-max_pre:-1], pre_in_cur[-1], cfg), (0, 1), 'constant', -0.1)
            merged = torch.cat([old, delta, last], 0)
            assert fed[-1].shape == merged.shape and torch.equal(fed[-1].view(torch.int32), merged.view(torch.int32)), f'frame {t}'
            want = sst_amd.FSD.simple_test(det, [merged], [dict(sample_idx=1003000 + t)])
            for g, w in zip(results[0], want[0]):
                assert torch.equal(getattr(g, 'tensor', g), getattr(w, 'tensor', w)), f'frame {t}'
            boxes = getattr(results[0][0], 'tensor', results[0][0])
            prev_pc.append(cur)
            prev_pose.append(pose)
            prev_seed.append(dict(boxes=boxes[:, :7].clone()))
            eb = R.enlarged(boxes, cfg['extra_width']) if len(boxes) else boxes
            prev_crop.append(cur[R.crop_indices(cur, eb, cap)])
            if len(prev_pc) > max_pre:
                for q in (prev_pc, prev_pose, prev_seed, prev_crop):
                    q.pop(0)
            lengths.append((len(det.previous_pc), len(det.previous_pose), len(det.previous_seed_info), len(det.previous_cropped_pc),
                            det.frame_counter))
            for mine, theirs in zip(prev_crop, det.previous_cropped_pc):
                assert torch.equal(mine, theirs)
        assert lengths == [(1, 1, 1, 1, 1), (2, 2, 2, 2, 2), (2, 2, 2, 2, 3), (2, 2, 2, 2, 4), (2, 2, 2, 2, 5)]
        assert any(len(getattr(s['gt_bboxes_3d'], 'tensor', s['gt_bboxes_3d'])) > 0 for s in det.previous_seed_info), 'no detections'
        # a new segment id resets the queues
        offline = seed_frames(clouds[5], 1, 40)
        det.simple_test([clouds[5].clone()], [dict(sample_idx=1004000)], seed_info=[[offline]], pose=[_pose(9)[None]])
        assert (len(det.previous_pc), len(det.previous_seed_info), len(det.previous_cropped_pc), det.frame_counter) == (1, 1, 1, 1)
        assert det.last_segind == '004'
