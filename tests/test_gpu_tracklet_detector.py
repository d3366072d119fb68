"""The CTRL tracklet detector on the GPU: configs/ctrl/ctrl_veh_24e.py (tests/golden/configs/ctrl) with sparse_shape cut to
[16, 64, 64] and the range cut to match, 3 tracklets of 5, 9 and 12 frames, about 40 points per frame, dropout 0.  forward_train
equals the same modules called step by step through torch indexing (tests/tracklet_ref.rows) and the reference-style targets
(tests/tracklet_ref.targets on the device): losses bit for bit, the logged IoU values within float32 rounding of their plain mean;
every parameter receives a finite gradient.  simple_test returns tracklets whose boxes equal roi_decode of the same predictions,
rows with an invalid RoI keeping their old box; the decoding variants equal the reference's (tests/golden/tracklet_train.npz)."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

import tracklet_ref as T
from test_configs_build import FIXTURES

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LENS = (5, 9, 12)
RANGE = [-6.4, -6.4, -1.6, 6.4, 6.4, 1.6]        # 64 x 64 x 16 voxels of 0.2 m


def small_model():
    model = eval(open(os.path.join(FIXTURES, 'ctrl', 'ctrl_veh_24e.model.py')).read())
    seg = model['segmentor']
    seg['voxel_layer']['point_cloud_range'] = seg['voxel_encoder']['point_cloud_range'] = seg['decode_neck']['point_cloud_range'] = RANGE
    seg['backbone']['sparse_shape'] = [16, 64, 64]
    model['roi_head']['bbox_head'].update(cls_dropout=0, reg_dropout=0)
    model['roi_head']['roi_extractor']['debug'] = True
    return model


def make_batch(seed):
    """-> (points, pts_frame_inds, tracklets, candidates_list) on the host: per tracklet a slow car near the origin, the prediction =
    its jittered boxes, ~40 points per frame inside the ground-truth box, two candidates (the path on most frames, a weaker copy)"""
    import sst_amd
    rng = np.random.default_rng(seed)
    points, frames, trks, cand_lists = [], [], [], []
    for t, n in enumerate(LENS):
        yaw = rng.uniform(-np.pi, np.pi) + np.cumsum(rng.normal(0, 0.01, n))
        xy = rng.uniform(-1.5, 1.5, 2) + np.cumsum(np.stack([np.sin(yaw), np.cos(yaw)], 1) * 0.08, 0)
        path = np.concatenate([xy, np.full((n, 1), -0.9), np.tile([1.9, 4.2, 1.6], (n, 1)), yaw[:, None]], 1).astype(np.float32)
        pred = T.jitter(rng, path, 0.6)
        ts = [T.TS0 + 100_000 * i for i in range(n)]
        trk = sst_amd.LiDARTracklet('seg', f'p{t}', 0, True, torch.as_tensor(pred), ts, rng.uniform(0.2, 0.9, n).astype(np.float32).tolist())
        trk.freeze()
        trk.set_type(0, 'mmdet3d')
        trk.pose_list = [torch.eye(4) for _ in range(n)]
        trk.shared_pose = torch.eye(4)
        keep = [i for i in range(n) if i != 1]
        cands = []
        for c, boxes in enumerate((path[keep], T.jitter(rng, path[keep], 2.0))):
            g = sst_amd.LiDARTracklet('seg', f'g{t}_{c}', 0, True, torch.as_tensor(boxes), [ts[i] for i in keep], [1.0] * len(keep))
            g.freeze()
            g.set_type(0, 'mmdet3d')
            cands.append(g)
        pts, fr = [], []
        for i in range(n):
            m = int(rng.integers(35, 46))
            local = (rng.random((m, 3)) - 0.5) * path[i, 3:6] * 0.95
            c, s = np.cos(path[i, 6]), np.sin(path[i, 6])
            # the box frame of this convention: the length lies along the heading (sin, cos)
            x = path[i, 0] + local[:, 0] * c + local[:, 1] * s
            y = path[i, 1] - local[:, 0] * s + local[:, 1] * c
            z = path[i, 2] + path[i, 5] / 2 + local[:, 2]
            deco = np.concatenate([rng.random((m, 2)), np.tile(np.r_[pred[i, 6], pred[i, 3:6], 0.5], (m, 1))], 1)      # 10 columns, as PointDecoration leaves them
            pts.append(np.concatenate([np.stack([x, y, z], 1), deco], 1))
            fr.append(np.full(m, i))
        p = np.concatenate(pts).astype(np.float32)
        p[:, :3] = np.clip(p[:, :3], np.asarray(RANGE[:3]) + 0.01, np.asarray(RANGE[3:]) - 0.01)
        order = rng.permutation(len(p))
        points.append(torch.as_tensor(p[order]))
        frames.append(torch.as_tensor(np.concatenate(fr)[order]).long())
        trks.append(trk)
        cand_lists.append(cands)
    return points, frames, trks, cand_lists


@pytest.fixture(scope='module')
def detector():
    import sst_amd
    torch.manual_seed(3)
    return sst_amd.build_detector(small_model()).to(DEV)


def on_device(batch):
    points, frames, trks, cand_lists = batch
    return [p.to(DEV) for p in points], [f.to(DEV) for f in frames], copy.deepcopy(trks), copy.deepcopy(cand_lists)


def test_forward_train_equals_the_modules_step_by_step(detector):
    import sst_amd
    det = detector.train()
    batch = make_batch(11)
    points, frames, trks, cand_lists = on_device(batch)
    det.zero_grad()
    losses = det.forward_train([p.clone() for p in points], frames, None, trks, cand_lists)
    total = losses['loss_rcnn_cls'] + losses['loss_rcnn_bbox'] + losses['loss_rcnn_corner']
    total.backward()
    missing = [k for k, p in det.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert not missing, missing
    assert float(losses['num_pos_rois']) > 10 and float(losses['num_neg_rois']) >= 3 and sorted(losses) == sorted(
        ['loss_rcnn_cls', 'loss_rcnn_bbox', 'loss_rcnn_corner', 'num_pos_rois', 'num_neg_rois', 'refined_iou', 'roi_iou', 'num_good',
         'num_good_rois'])

    # the same step, module by module
    _, _, trks2, cands2 = on_device(batch)
    head = det.roi_head
    seg = det.segmentor.forward_train([p.clone() for p in points], frames, None)
    cfg = dict(candidate_thresh=0.5, object_centric=False, iou_thr=0.5, cls_pos_thr=(0.8,), cls_neg_thr=(0.2,), num_classes=1)
    as_trk = lambda t: T.Trk(t.boxes.to(DEV), t.ts_list, t.score_list, 0)        # noqa: E731
    ref = T.targets([as_trk(t) for t in trks2], [[as_trk(c) for c in cs] for cs in cands2], cfg, torch.float32,
                    iou_fn=sst_amd.aligned_iou_3d)
    ref = {k: v.to(DEV) for k, v in ref.items()}
    rois = ref['rois'].contiguous()
    xyz = seg['seg_points'][:, :3]
    inds, roi_inds, info = head.roi_extractor(xyz, seg['batch_idx'], seg['pts_frame_inds'], rois, ref['frame_inds'])
    feats, new_xyz = T.rows(seg['seg_feats'], xyz, seg['pts_frame_inds'], inds, roi_inds, ref['frame_inds'], ref['scores'], True, True)
    cls_score, bbox_pred, valid = head.bbox_head(new_xyz, feats, info, roi_inds, rois)
    ref['gts'] = torch.cat([c.boxes for cs in cands2 for c in cs]).to(DEV)
    step = head.bbox_head.loss(cls_score, bbox_pred, valid, rois, ref)
    for k in ('loss_rcnn_cls', 'loss_rcnn_bbox', 'loss_rcnn_corner', 'num_pos_rois', 'num_neg_rois'):
        print(k, float(losses[k].detach()), float(step[k].detach()))
        assert torch.equal(losses[k].detach(), step[k].detach()), k
    pos = ref['reg_mask'] > 0
    decoded = sst_amd.roi_head.roi_decode(rois, bbox_pred.detach().contiguous(), with_bev=False)[0]
    for name, good, boxes in (('refined_iou', 'num_good', decoded), ('roi_iou', 'num_good_rois', rois[:, 1:])):
        ious = sst_amd.aligned_iou_3d(ref['pos_gt_bboxes'][pos].contiguous(), boxes[pos].contiguous())
        print(name, float(losses[name]), float(ious.mean()), good, float(losses[good]), int((ious > 0.7).sum()))
        assert abs(float(losses[name]) - float(ious.double().mean())) <= 1e-6 and float(losses[good]) == float((ious > 0.7).sum())


def test_simple_test_updates_the_tracklets_from_roi_decode(detector):
    import sst_amd
    det = detector.eval()
    batch = make_batch(12)
    points, frames, trks, cand_lists = on_device(batch)
    _, _, before, _ = on_device(batch)
    with torch.no_grad():
        out = det.simple_test([p.clone() for p in points], None, frames, trks, cand_lists)
        # the same predictions, by hand
        head = det.roi_head
        for t in before:
            t.to(DEV)
        seg = det.segmentor.simple_test([p.clone() for p in points], frames, None)
        rois, roi_frame_inds, cls_preds, labels_3d = head.tracklets2rois(before)
        res = head._bbox_forward(seg['seg_points'][:, :3], seg['seg_feats'], seg['batch_idx'], seg['pts_frame_inds'], rois, cls_preds,
                                 roi_frame_inds)
        boxes, scores, _ = sst_amd.roi_head.roi_decode(rois, res['bbox_pred'].contiguous(), res['cls_score'].contiguous(), with_bev=False)
    assert len(out) == 3 and all(a is b for a, b in zip(out, trks))
    valid = res['valid_roi_mask'].cpu()
    r0 = 0
    for t, old in zip(out, before):
        n = len(old)
        sl = slice(r0, r0 + n)
        new_ego, old_ego = old.shared2ego(boxes[sl]).cpu(), old.shared2ego().cpu()
        expected = torch.where(valid[sl, None], new_ego, old_ego)
        assert torch.equal(t.concated_boxes().cpu(), expected) and t.pose_list is None
        exp_scores = torch.where(valid[sl], scores[sl].cpu(), torch.tensor(old.score_list))
        assert torch.equal(torch.tensor(t.score_list), exp_scores)
        r0 += n
    assert bool(valid.any())
    # a RoI without any point is invalid and keeps its old box: move one tracklet's points away
    points2, frames2, trks2, _ = on_device(batch)
    far = points2[1].clone()
    far[:, :2] = far[:, :2].clamp(min=5.9)
    old1 = copy.deepcopy(trks2[1]).to(DEV)
    with torch.no_grad():
        out2 = det.simple_test([points2[0], far, points2[2]], None, frames2, trks2, None)
    assert torch.equal(out2[1].concated_boxes().cpu(), old1.shared2ego().cpu())
    assert out2[1].score_list == pytest.approx(old1.score_list, abs=0, rel=1e-7)


def test_decoding_variants_equal_the_reference():
    import sst_amd
    gold = load_golden('tracklet_train.npz')
    dev = lambda x, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(x)).to(dt).to(DEV)        # noqa: E731
    rois, gt_rois = dev(gold['oc1_rois_f64']), dev(gold['oc1_gt_rois_f64'])
    args = (rois, dev(gold['cls_score']), dev(gold['bbox_pred']), dev(gold['roi_valid'], torch.bool), dev(gold['oc1_labels_3d'], torch.long),
            dev(gold['oc1_cls_preds_f64']))
    for name, cfg in (('plain', {}), ('replace', dict(replace_center=True, replace_size=True, replace_yaw=True))):
        res = sst_amd.get_bboxes_from_tracklet(*args, None, gt_rois=gt_rois, cfg=cfg)
        assert [len(r[0]) for r in res] == gold['lens'].tolist()
        boxes, scores = torch.cat([r[0] for r in res]).cpu().numpy(), torch.cat([r[1] for r in res]).cpu().numpy()
        for got, key in ((boxes, f'decode_{name}_boxes'), (scores, f'decode_{name}_scores')):
            err, gap = T.rel_err(got, gold[key + '_f64']), float(gold['noise_' + key])
            print(key, 'err', err, 'gap', gap)
            assert err <= T.bar(gap)
        assert torch.equal(torch.cat([r[3] for r in res]).cpu(), torch.as_tensor(gold['roi_valid']))
    res = sst_amd.get_bboxes_from_tracklet(*args, None, gt_rois=gt_rois, cfg=dict(identical_decode=True), batch_size=8)
    assert torch.equal(torch.cat([r[0] for r in res]), rois[:, 1:]) and torch.equal(torch.cat([r[1] for r in res]), args[5])
