"""Generates tests/golden/tracklet_tta.npz and tests/golden/configs/pipeline/ctrl/ctrl_{veh_24e,ped_24e,cyc_12e}.tta_pipeline.py: the
CTRL test-time augmentation as the REFERENCE computes it, view by view (data only: arrays in the .npz, literal dicts in the
fixtures).

Needs the reference tree (oracle.ref_loader); run from the repository root:  python tests/golden/make_tracklet_tta.py

Executed from their source text: MultiScaleFlipAug3D (mmdet3d/datasets/pipelines/test_time_aug.py), TrackletPoseTransform,
PointDecoration, TrackletGlobalRotScaleTrans and TrackletRandomFlip (tracklet_pipelines.py), PointsRangeFilter and PointShuffle
(transforms_3d.py), TrackletRoIHead.inverse_aug (mmdet3d/models/roi_heads/tracklet_roi_head.py), LiDARTracklet with
update_from_prediction, shared2ego and merge_augs in its three modes (core/bbox/structures/lidar_tracklet.py), LiDARPoints and
LiDARInstance3DBoxes as tests/golden/make_tracklet_pipeline.py and make_tracklet.py load them.  Stand-ins: ``Compose`` builds the
transforms above from their dicts, skips TrackletFormatBundle and Collect3D, and records the points, the range mask and the boxes
of every view in front of PointsRangeFilter; ``mmcv.is_list_of``; ``np.float`` (removed from numpy) reads ``float``; TorchEx
boxes_overlap_1to1 is the diagonal of tests/box_ops_ref.py.  Every case runs in float32 and in float64 on the same inputs; gap_*
is the difference between the two runs relative to the largest element.

The inputs are make_tracklet_pipeline.py's three tracklets (1, 37 and 160 frames, empty frames, world poses 10^4 m from the
origin).  The decoded boxes of a view are its augmented boxes plus a jitter that grows with the view, so that the IoU against
view 0 falls on both sides of iou_merge_thresh; some rows are jittered far enough that every view but the first is clamped; the
valid masks have rows that are invalid in some and in all views; two views of one case carry equal scores on some rows (ties for
'max').  Points whose reference output lies within 1e-3 m of a range bound in any view are taken out; a decoded box whose IoU
lies within 1e-4 of iou_merge_thresh is replaced by the view's own box (IoU 1 after the round trip); it is asserted that none is
left and that at most 5 % were taken out."""
import copy
import os
import pprint
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'tests'), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import box_ops_ref as B  # noqa: E402
import tracklet_ref as T  # noqa: E402
from tracklet_tta_ref import GOLDEN_CASES as CASES  # noqa: E402
import make_roi_head_train as M  # noqa: E402
import make_tracklet_pipeline as P  # noqa: E402

TTA_PY = 'mmdet3d/datasets/pipelines/test_time_aug.py'
ROI_PY = 'mmdet3d/models/roi_heads/tracklet_roi_head.py'
THRESH = 0.55
IOU_MARGIN = 1e-4
PROPS = ['yaw', 'size', 'score']
MODES = ('max', 'weighted', 'iou_clamped_weighted')
SKIPPED = ('TrackletFormatBundle', 'Collect3D')


class NpCompat(object):
    """``np`` with the alias numpy removed"""
    float = float

    def __getattr__(self, name):
        return getattr(np, name)


def is_list_of(seq, expected_type):
    return isinstance(seq, list) and all(isinstance(x, expected_type) for x in seq)


def reference(f64):
    """the reference's classes -> dict (make_tracklet_pipeline.reference plus the test-time pieces)"""
    import torch.nn.functional as F
    from oracle import ref_loader as L
    ref = P.reference(f64)
    lidar = ref['lidar']
    npdt = np.float64 if f64 else np.float32
    tm = P.TorchProxy(ref['log'], f64)

    def boxes_overlap_1to1(a, b):
        ra, rb = a.numpy().astype(npdt), b.numpy().astype(npdt)
        if f64:
            return torch.as_tensor(np.array([B.bev_overlap_f64(x, y) for x, y in zip(ra, rb)], np.float64).reshape(-1))
        return torch.as_tensor(B.bev_overlap_f32(ra, rb).astype(np.float32))

    lidar.aligned_iou_3d.__func__.__globals__['boxes_overlap_1to1'] = boxes_overlap_1to1
    ref['tracklet'] = L.load_reference_class(P.TRK_PY, 'LiDARTracklet', dict(np=NpCompat(), torch=tm, F=F, LiDARInstance3DBoxes=lidar,
                                                                             copy=copy))
    ref['inverse_aug'] = L.load_reference_method(ROI_PY, 'TrackletRoIHead', 'inverse_aug', dict(torch=tm))

    class Compose(object):
        def __init__(self, transforms):
            self.steps = []
            for t in transforms:
                t = dict(t)
                name = t.pop('type')
                if name not in SKIPPED:
                    self.steps.append((name, ref[name](**t)))

        def __call__(self, d):
            rec = {}
            for name, fn in self.steps:
                if name == 'PointsRangeFilter':
                    rec['xyz'] = d['points'].tensor[:, :3].numpy().copy()
                    rec['mask'] = d['points'].in_range_3d(fn.pcd_range).numpy().copy()
                    rec['boxes'] = P.cat_boxes(d['tracklet'])
                    rec['frame_inds'] = d['pts_frame_inds'].numpy().astype(np.int64)
                    before = d['points'].tensor.numpy().copy()
                d = fn(d)
                if name == 'PointsRangeFilter':
                    rec['final'] = d['points'].tensor.numpy().copy()
                    rec['final_frame_inds'] = d['pts_frame_inds'].numpy().astype(np.int64)
                    assert np.array_equal(rec['final'], before[rec['mask']])
                if name == 'PointShuffle':
                    s, f = d['points'].tensor.numpy(), rec['final']
                    assert np.array_equal(s[np.lexsort(s.T[::-1])], f[np.lexsort(f.T[::-1])])          # a permutation
            d['_rec'] = rec
            return d

    ref['MultiScaleFlipAug3D'] = L.load_reference_class(TTA_PY, 'MultiScaleFlipAug3D', dict(
        mmcv=types.SimpleNamespace(is_list_of=is_list_of), warnings=warnings, deepcopy=copy.deepcopy, Compose=Compose))
    return ref


def tta_step(case):
    return dict(type='MultiScaleFlipAug3D', img_scale=(1333, 800), pts_scale_ratio=1, pts_rots=case['rots'], flip=case['flip'],
                pcd_horizontal_flip=case['h'], pcd_vertical_flip=case['v'],
                transforms=[dict(type='TrackletGlobalRotScaleTrans', rot_range=[0, 0], scale_ratio_range=[1.0, 1.0], translation_std=[0, 0, 0]),
                            dict(type='TrackletRandomFlip', flip_ratio_bev_horizontal=0.0, flip_ratio_bev_vertical=0.0),
                            dict(type='PointsRangeFilter', point_cloud_range=P.RANGE), dict(type='PointShuffle'),
                            dict(type='TrackletFormatBundle', class_names=['Car']),
                            dict(type='Collect3D', keys=['points', 'pts_frame_inds', 'tracklet'])])


def run_views(ref, inp, case, keep):
    """the reference's tta chain on one tracklet -> (arrays, the per-view tracklets, the per-view metas)"""
    log = ref['log']
    del log[:]
    np.random.seed(5)
    dt = ref['dtype']
    frames = [f if keep is None else f[keep[k]] for k, f in enumerate(inp['frames'])]
    trk = P.build_tracklet(ref, inp['boxes'], inp['ts'], inp['scores'], inp['ts2pose'], 'p')
    trk.set_type(0, 'mmdet3d')
    d = dict(tracklet=trk, points=[torch.from_numpy(f.copy()).to(dt) for f in frames],
             pts_frame_inds=[torch.ones(len(f), dtype=torch.int) * i for i, f in enumerate(frames)])
    center = trk.pose_list[len(trk.pose_list) // 2]
    out = dict(mm=torch.stack([torch.linalg.inv(center) @ p for p in trk.pose_list]).numpy())
    d = ref['TrackletPoseTransform'](concat=False)(d)
    out['pose_boxes'] = P.cat_boxes(trk)
    out['shared_pose'] = trk.shared_pose.numpy()
    d = ref['PointDecoration'](properties=PROPS, concat=True)(d)
    full = d['points'].tensor.numpy()
    lens = np.asarray([len(f) for f in frames], np.int64)
    first = np.concatenate([[0], np.cumsum(lens)])[:-1]
    out['deco'] = np.array([full[first[k], 5:] if lens[k] else np.full(full.shape[1] - 5, np.nan) for k in range(len(lens))])
    aug = ref['MultiScaleFlipAug3D'](**{k: v for k, v in tta_step(case).items() if k != 'type'})(d)
    K = len(aug['points'])
    assert [k for k, _ in log].count('normal') == K          # the zero-std translation is drawn once per view
    assert all(np.array_equal(np.asarray(t), np.zeros(3)) and not np.signbit(np.asarray(t)).any() for t in aug['pcd_trans'])
    out['view_table'] = np.array([[float(aug['pcd_horizontal_flip'][k]), float(aug['pcd_vertical_flip'][k]), float(aug['pcd_rot_angle'][k])]
                                  for k in range(K)], np.float64)
    recs = aug['_rec']
    out['xyz'] = np.stack([r['xyz'] for r in recs])
    out['masks'] = np.stack([r['mask'] for r in recs])
    out['aug_boxes'] = np.stack([r['boxes'] for r in recs])
    out['frame_inds'] = recs[0]['frame_inds']
    out['final_frame_inds'] = np.concatenate([r['final_frame_inds'] for r in recs])
    metas = [dict(pcd_horizontal_flip=aug['pcd_horizontal_flip'][k], pcd_vertical_flip=aug['pcd_vertical_flip'][k],
                  pcd_rot_angle=aug['pcd_rot_angle'][k]) for k in range(K)]
    return out, aug['tracklet'], metas


def predictions(rng, aug_boxes, n_case):
    """the decoded boxes, scores and valid masks of every view, from the float32 run's augmented boxes"""
    K, n = aug_boxes.shape[:2]
    pred = np.stack([T.jitter(rng, aug_boxes[k].astype(np.float32), 0.15 + 0.25 * (k % 5)) for k in range(K)]).astype(np.float32)
    far = rng.random(n) < 0.12
    if n > 3:
        far[3] = True
    for k in range(1, K):                                   # every view but the first leaves view 0's box there
        pred[k, far, :2] += np.float32(3.0)
    scores = rng.uniform(0.05, 0.95, (K, n)).astype(np.float32)
    valid = rng.random((K, n)) < 0.8
    valid[:, 0] = True
    if n > 2:
        valid[:, 1] = False
        valid[:, 2] = np.arange(K) % 2 == 0
    if n == 1 and n_case == 0:
        valid[K - 1, 0] = False
    if K > 2 and n > 5:                                     # ties for 'max': the first of two equal maxima wins
        scores[2, 4:8] = scores[1, 4:8] = np.float32(0.97)
        valid[1:3, 4:8] = True
    return pred, scores, valid


def run_finish(ref, view_trks, metas, pred, scores, valid):
    """inverse_aug and update_from_prediction per view, then merge_augs in its three modes -> dict"""
    dt = ref['dtype']
    K, n = scores.shape
    trks = []
    for k in range(K):
        trk = copy.deepcopy(view_trks[k])
        boxes = ref['lidar'](torch.as_tensor(pred[k]).to(dt))
        ref['inverse_aug'](None, trk, boxes, metas[k])
        trk.update_from_prediction(boxes, torch.as_tensor(scores[k]), torch.zeros(n, dtype=torch.long), torch.as_tensor(valid[k]))
        assert trk.pose_list is None
        trks.append(trk)
    out = dict(ego=np.stack([np.concatenate(t.box_list, 0) for t in trks]), ego_scores=np.array([t.score_list for t in trks], np.float64))
    flat = ref['lidar'](out['ego'].reshape(K * n, 7))
    base = ref['lidar'](np.concatenate([out['ego'][0]] * K, 0))
    out['ious'] = ref['lidar'].aligned_iou_3d(base, flat).reshape(K, n).numpy()
    for mode in MODES:
        merged = ref['tracklet'].merge_augs([copy.deepcopy(t) for t in trks], dict(merge=mode, iou_merge_thresh=THRESH), 'cpu')
        out[f'merged_{mode}_boxes'] = np.concatenate(merged.box_list, 0)
        out[f'merged_{mode}_scores'] = np.asarray(merged.score_list, np.float64)
    return out


def tta_fixtures():
    from oracle import ref_loader
    from sst_amd.optim import resolve_config
    dst = os.path.join(ROOT, 'tests', 'golden', 'configs', 'pipeline', 'ctrl')
    os.makedirs(dst, exist_ok=True)
    for name in ('ctrl_veh_24e', 'ctrl_ped_24e', 'ctrl_cyc_12e'):
        path = os.path.join(ref_loader.REF_ROOT, 'configs', 'ctrl', name + '.py')
        cfg = resolve_config(open(path).read(), os.path.dirname(path), path)
        with open(os.path.join(dst, name + '.tta_pipeline.py'), 'w') as f:
            f.write(pprint.pformat({'tta_pipeline': cfg['tta_pipeline']}, width=120) + '\n')


def main():
    from oracle import ref_loader
    if not ref_loader.available():
        raise SystemExit('the reference tree is not present')
    r32, r64 = reference(False), reference(True)
    inputs = P.make_inputs()
    out = dict(range=np.asarray(P.RANGE, np.float64), n_cases=np.int64(len(CASES)), iou_merge_thresh=np.float64(THRESH))
    taken = total = 0
    for c, case in enumerate(CASES):
        inp = inputs[case['trk']]
        rng = np.random.default_rng(900 + c)
        with M.patched(False):
            first, _, _ = run_views(r32, inp, case, None)
            bad = np.zeros(first['xyz'].shape[1], bool)
            for k in range(first['xyz'].shape[0]):
                bad |= P.near_bound(first['xyz'][k])
            keep, at = [], 0
            for fr in inp['frames']:
                keep.append(~bad[at:at + len(fr)])
                at += len(fr)
            res, trks32, metas = run_views(r32, inp, case, keep)
            assert not any(P.near_bound(x).any() for x in res['xyz'])
            pred, scores, valid = predictions(rng, res['aug_boxes'], c)
            fin = run_finish(r32, trks32, metas, pred, scores, valid)
            near = np.abs(fin['ious'].astype(np.float64) - THRESH) < IOU_MARGIN
            near[0] = False
            pred[near] = res['aug_boxes'][near]
            fin = run_finish(r32, trks32, metas, pred, scores, valid)
            near2 = np.abs(fin['ious'].astype(np.float64) - THRESH) < IOU_MARGIN
            near2[0] = False
            assert not near2.any()
            taken += int(bad.sum()) + int(near.sum())
            total += len(bad) + near.size
        with M.patched(True):
            res64, trks64, metas64 = run_views(r64, inp, case, keep)
            fin64 = run_finish(r64, trks64, metas64, pred, scores, valid)
        assert np.array_equal(res['masks'], res64['masks'])
        # the float64 run may clamp other views (the ego boxes of the two runs differ by the poses' float32 error, far more than
        # the IoU margin): recorded, and gap_merged_iou_clamped_* is then the gap of two different sums
        out[f'c{c}_iou_mask_agrees'] = np.bool_(np.array_equal(fin['ious'][1:] > np.float32(THRESH), fin64['ious'][1:] > THRESH))
        K = len(metas)
        kept_frames = [f[m] for f, m in zip(inp['frames'], keep)]
        res.update(fin)
        res.update(points=np.concatenate(kept_frames), frame_lens=np.asarray([len(f) for f in kept_frames], np.int64),
                   boxes=inp['boxes'], ts=np.asarray(inp['ts'], np.int64), scores=np.asarray(inp['scores'], np.float64),
                   poses=np.stack([inp['ts2pose'][ts] for ts in inp['ts']]), pred=pred, pred_scores=scores, valid=valid,
                   counts=res['masks'].sum(1).astype(np.int64))
        for key in ('mm', 'pose_boxes', 'xyz', 'aug_boxes'):
            out[f'c{c}_gap_{key}'] = np.float64(P.rel(res[key], res64[key]))
        for key in ['ego'] + [f'merged_{m}_{w}' for m in MODES for w in ('boxes', 'scores')]:
            out[f'c{c}_gap_{key}'] = np.float64(P.rel(fin[key], fin64[key]))
        if K > 5:
            del res['xyz']                                   # the masks and the frame indices pin the views of the wide cases
        f64_keys = ('view_table', 'scores', 'ego_scores') + tuple(f'merged_{m}_{w}' for m in MODES for w in ('boxes', 'scores'))
        for key, v in res.items():
            v = np.asarray(v)
            out[f'c{c}_{key}'] = v.astype(np.float32) if v.dtype == np.float64 and key not in f64_keys else v
        inv_rows = int((~valid).all(0).sum())
        clamp_rows = int(((fin['ious'][1:] <= THRESH).all(0)).sum()) if K > 1 else 0
        print('case', c, 'frames', len(inp['ts']), 'views', K, 'points', res['masks'].shape[1], 'kept', res['counts'].tolist()[:6],
              'rows invalid in every view', inv_rows, 'rows clamped to view 0', clamp_rows,
              'gap ego', float(out[f'c{c}_gap_ego']), 'gap weighted', float(out[f'c{c}_gap_merged_weighted_boxes']))
    assert taken <= 0.05 * total, (taken, total)
    out['taken_out'] = np.asarray([taken, total], np.int64)
    path = os.path.join(ROOT, 'tests', 'golden', 'tracklet_tta.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes', len(out), 'arrays; taken out', taken, 'of', total)
    assert os.path.getsize(path) < 700 * 1024
    tta_fixtures()


if __name__ == '__main__':
    main()
