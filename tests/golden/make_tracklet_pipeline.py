"""Generates tests/golden/tracklet_pipeline.npz and tests/golden/configs/pipeline/ctrl/ctrl_{veh_24e,ped_24e,cyc_12e}.pipeline.py:
the CTRL tracklet pipeline as the REFERENCE computes it, stage by stage (data only: arrays in the .npz, literal dicts in the
fixtures).

Needs the reference tree (oracle.ref_loader); run from the repository root:  python tests/golden/make_tracklet_pipeline.py

Executed from their source text: TrackletCutting, TrackletPoseTransform, TrackletNoise, PointDecoration, TrackletRandomFlip and
TrackletGlobalRotScaleTrans (mmdet3d/datasets/pipelines/tracklet_pipelines.py), PointsRangeFilter and PointShuffle
(transforms_3d.py), BasePoints and LiDARPoints (core/points), LiDARTracklet (core/bbox/structures/lidar_tracklet.py) and
LiDARInstance3DBoxes as tests/golden/make_tracklet.py loads it.  Stand-ins: ``get_points_type`` returns LiDARPoints; ``np`` and
``torch`` are read through recorders that log every ``np.random`` / ``torch.rand`` draw and otherwise pass everything on.  Every
case runs in float32 and in float64 (``torch.float32`` read as ``torch.float64``, the ``torch.rand`` draws made in float32 and
widened, so that both runs see the same numbers); gap_* is the difference between the two runs relative to the largest element.
The per-frame matrices ``mm`` are the reference's own expression, ``torch.linalg.inv(center_pose) @ pose`` frame by frame
(tracklet_pipelines.py:167, :206), evaluated here because the transform does not hand them out.

The cases: tracklets of 1, 37 and 160 frames (the last above max_length = 150: the cut runs) with 0, 1 and 2 candidates whose
timestamps reach outside their tracklet; 0 to 80 points per frame with empty frames; world poses with translations of 10^4 m;
flips (0, 0), (1, 0), (0, 1) and - the 37-frame tracklet once more - (1, 1); consistent centre and size noise on cases 0 and 3
(the yaw noise is never consistent here: lidar_tracklet.py:542 adds a [1] tensor to a 0-d element in place, which torch refuses).  Inputs whose
reference output lies within 1e-3 m of a range bound are taken out, and it is asserted that none is left.  Every tracklet also
runs through the test pipeline (no cut, noise, flip, rotation; no candidates)."""
import copy
import os
import pprint
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'tests'), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import tracklet_ref as T  # noqa: E402
import make_roi_head_train as M  # noqa: E402

PIPE_PY = 'mmdet3d/datasets/pipelines/tracklet_pipelines.py'
T3D_PY = 'mmdet3d/datasets/pipelines/transforms_3d.py'
TRK_PY = 'mmdet3d/core/bbox/structures/lidar_tracklet.py'
RANGE = [-24.0, -24.0, -2.5, 24.0, 24.0, 3.0]
MARGIN = 1e-3
NOISE = dict(center=[0.2, 0.2, 0.1], size=[0.2, 0.2, 0.1], yaw=0.2)
CUT = dict(ratio=0.0, max_length=150)
RST = dict(rot_range=[-0.78539816, 0.78539816], scale_ratio_range=[0.95, 1.05], translation_std=[0, 0, 0.2])
CASES = [dict(trk=0, flips=(0, 0), consistent=True, seed=11), dict(trk=1, flips=(1, 0), consistent=False, seed=12),
         dict(trk=2, flips=(0, 1), consistent=False, seed=13), dict(trk=1, flips=(1, 1), consistent=True, seed=14)]
LENS, N_CANDS, KINDS = [1, 37, 160], [0, 1, 2], [0, 1, 2]
PROPS = ['yaw', 'size', 'score', 'length']


class Log(list):
    pass


class NpRandom(object):
    """np.random with every draw logged"""

    def __init__(self, log):
        self.log = log

    def _draw(self, name, *a, **k):
        v = getattr(np.random, name)(*a, **k)
        self.log.append((name, np.array(v, np.float64).copy()))
        return v

    def rand(self, *a, **k):
        return self._draw('rand', *a, **k)

    def randint(self, *a, **k):
        return self._draw('randint', *a, **k)

    def uniform(self, *a, **k):
        return self._draw('uniform', *a, **k)

    def normal(self, *a, **k):
        return self._draw('normal', *a, **k)


class NpProxy(object):
    def __init__(self, log):
        self.random = NpRandom(log)

    def __getattr__(self, name):
        return getattr(np, name)


class TorchProxy(object):
    """``torch`` with ``rand`` logged (drawn in float32 in both runs); in the float64 run float32 and float read as float64"""

    def __init__(self, log, f64):
        self.log, self.f64 = log, f64

    def rand(self, *size, dtype=None, device=None, **k):
        v = torch.rand(*size, dtype=torch.float32, **k)
        self.log.append(('torch.rand', v.numpy().copy()))
        return v.double() if self.f64 else v

    def __getattr__(self, name):
        if self.f64 and name in ('float32', 'float'):
            return torch.float64
        return getattr(torch, name)


def reference(f64):
    """the reference's classes under the recorders -> dict"""
    from abc import abstractmethod
    import warnings
    import torch.nn.functional as F
    from oracle import ref_loader as L
    log = Log()
    npx, tm = NpProxy(log), TorchProxy(log, f64)
    lidar = M.reference_parts(f64)['lidar']
    base_points = L.load_reference_class('mmdet3d/core/points/base_points.py', 'BasePoints',
                                         dict(np=np, torch=tm, abstractmethod=abstractmethod, warnings=warnings))
    lidar_points = L.load_reference_class('mmdet3d/core/points/lidar_points.py', 'LiDARPoints', dict(torch=tm, BasePoints=base_points))
    lidar_points.__init__.__globals__['LiDARPoints'] = lidar_points
    trk = L.load_reference_class(TRK_PY, 'LiDARTracklet', dict(np=np, torch=tm, F=F, LiDARInstance3DBoxes=lidar, copy=copy))
    glb = dict(np=npx, torch=tm, F=F, BasePoints=base_points, LiDARInstance3DBoxes=lidar, get_points_type=lambda name: lidar_points)
    out = dict(log=log, lidar=lidar, points=lidar_points, tracklet=trk, dtype=torch.float64 if f64 else torch.float32, f64=f64)
    for name in ('TrackletCutting', 'TrackletPoseTransform', 'TrackletNoise', 'PointDecoration', 'TrackletRandomFlip',
                 'TrackletGlobalRotScaleTrans'):
        out[name] = L.load_reference_class(PIPE_PY, name, dict(glb))
    for name in ('PointsRangeFilter', 'PointShuffle'):
        out[name] = L.load_reference_class(T3D_PY, name, dict(np=np, torch=tm))
    return out


def world_pose(rng, origin, heading, k):
    """the ego pose of frame k: 1.2 m per frame along a slowly turning heading, 10^4 m from the world origin"""
    a = heading + 0.004 * k
    m = np.eye(4)
    m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    m[:3, 3] = origin + np.array([np.cos(heading) * 1.2 * k, np.sin(heading) * 1.2 * k, 0.01 * k])
    return m.astype(np.float32)


def make_inputs():
    """three tracklets with their candidates, poses by timestamp and per-frame points (5 columns) -> list of dicts"""
    rng = np.random.default_rng(20261021)
    trks, cand_lists = T.make_tracklets(77, LENS, N_CANDS, KINDS)
    out = []
    for t, (trk, cands) in enumerate(zip(trks, cand_lists)):
        n = len(trk.ts_list)
        all_ts = sorted(set(trk.ts_list) | {x for c in cands for x in c.ts_list})
        origin = np.array([1.0e4 + 300 * t, -2.0e4 - 100 * t, 35.0])
        heading = rng.uniform(-np.pi, np.pi)
        ts2pose = {ts: world_pose(rng, origin, heading, (ts - T.TS0) // 100_000 - 7 * t) for ts in all_ts}
        boxes = trk.boxes.numpy().copy()
        boxes[:, :2] = boxes[:, :2] * 0.3                      # the object within some metres of the ego vehicle
        for c in cands:
            c.boxes = torch.as_tensor(np.concatenate([c.boxes.numpy()[:, :2] * 0.3, c.boxes.numpy()[:, 2:]], 1).astype(np.float32))
        lens = np.where(rng.random(n) < (0.15 if n < 100 else 0.04), rng.integers(60, 81, n), rng.integers(0, 20 if n < 100 else 9, n))
        lens[rng.random(n) < 0.1] = 0
        if n == 1:
            lens[:] = 57
        if n > 10:
            lens[0], lens[5], lens[n - 1] = 0, 80, 0
        frames = []
        for k in range(n):
            p = np.zeros((lens[k], 5), np.float32)
            p[:, :3] = boxes[k, :3] + rng.uniform(-1, 1, (lens[k], 3)) * [14.0, 14.0, 2.2]
            p[:, 3:] = rng.uniform(0, 1, (lens[k], 2))
            frames.append(p)
        out.append(dict(boxes=boxes.astype(np.float32), ts=list(trk.ts_list), scores=[float(s) for s in trk.score_list], kind=KINDS[t],
                        frames=frames, cands=[dict(boxes=c.boxes.numpy().copy(), ts=list(c.ts_list)) for c in cands], ts2pose=ts2pose))
    return out


def build_tracklet(ref, boxes, ts, scores, ts2pose, name):
    b = np.asarray(boxes, np.float32)
    t = ref['tracklet']('seg', name, 1, True, [b[i:i + 1].copy() for i in range(len(b))], list(ts), list(scores))
    t.freeze()
    t.set_poses({k: torch.as_tensor(v).to(ref['dtype']) for k, v in ts2pose.items()})
    return t


def cat_boxes(trk):
    return np.concatenate([b.tensor.numpy() for b in trk.box_list], 0) if len(trk.box_list) else np.zeros((0, 7))


def run_train(ref, inp, case, keep=None):
    """the reference's train chain on one tracklet -> arrays after every stage; ``keep``: per frame the rows to keep"""
    log = ref['log']
    del log[:]
    np.random.seed(case['seed'])
    torch.manual_seed(case['seed'])
    dt = ref['dtype']
    frames = [f if keep is None else f[keep[k]] for k, f in enumerate(inp['frames'])]
    trk = build_tracklet(ref, inp['boxes'], inp['ts'], inp['scores'], inp['ts2pose'], 'p')
    cands = [build_tracklet(ref, c['boxes'], c['ts'], [1.0] * len(c['ts']), inp['ts2pose'], f'c{j}') for j, c in enumerate(inp['cands'])]
    d = dict(tracklet=trk, gt_tracklet_candidates=cands, points=[torch.from_numpy(f.copy()).to(dt) for f in frames],
             pts_frame_inds=[torch.ones(len(f), dtype=torch.int) * i for i, f in enumerate(frames)],
             pcd_horizontal_flip=bool(case['flips'][0]), pcd_vertical_flip=bool(case['flips'][1]))
    out = {}
    d = ref['TrackletCutting'](**CUT)(d)
    out['cut_ts'] = np.asarray(trk.ts_list, np.int64)
    out['cut_frame_values'] = np.asarray([int(v[0]) if len(v) else -1 for v in d['pts_frame_inds']], np.int64)
    out['cut_scores'] = np.asarray(trk.score_list, np.float64)
    out['cut_boxes'] = cat_boxes(trk)
    out['cut_index'] = np.asarray([trk.ts2index[ts] for ts in trk.ts_list], np.int64)
    out['cut_lens'] = np.asarray([len(p) for p in d['points']], np.int64)
    center = trk.pose_list[len(trk.pose_list) // 2]
    inv = torch.linalg.inv(center)
    out['mm'] = torch.stack([inv @ p for p in trk.pose_list]).numpy()
    out['cand_mm'] = [torch.stack([inv @ p for p in c.pose_list]).numpy() for c in cands]
    d = ref['TrackletPoseTransform'](concat=False)(d)
    out['pose_points'] = torch.cat(d['points'], 0)[:, :3].numpy()
    out['pose_boxes'] = cat_boxes(trk)
    out['cand_pose_boxes'] = [cat_boxes(c) for c in cands]
    cons = case['consistent']
    d = ref['TrackletNoise'](center_noise_cfg=dict(max_noise=NOISE['center'], consistent=cons),
                             size_noise_cfg=dict(max_noise=NOISE['size'], consistent=cons),
                             yaw_noise_cfg=dict(max_noise=NOISE['yaw'], consistent=False))(d)
    rands = [v for k, v in log if k == 'torch.rand']
    out['u_center'], out['u_size'], out['u_yaw'] = rands[-3:]
    out['noise_boxes'] = cat_boxes(trk)
    d = ref['PointDecoration'](properties=PROPS, concat=True)(d)
    full = d['points'].tensor.numpy()
    lens = out['cut_lens']
    first = np.concatenate([[0], np.cumsum(lens)])[:-1]
    rows = np.array([full[first[k], 5:] if lens[k] else np.full(full.shape[1] - 5, np.nan) for k in range(len(lens))])
    of = np.repeat(np.arange(len(lens)), lens)
    assert np.array_equal(full[:, 5:], rows[of])                     # one set of values per frame
    out['deco'] = rows
    out['frame_inds'] = d['pts_frame_inds'].numpy().astype(np.int64)
    d = ref['TrackletRandomFlip'](flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5)(d)
    out['flip_points'], out['flip_boxes'] = d['points'].tensor[:, :3].numpy().copy(), cat_boxes(trk)
    out['cand_flip_boxes'] = [cat_boxes(c) for c in cands]
    rst = ref['TrackletGlobalRotScaleTrans'](**RST)
    rst._random_rot(d)
    rst._rot_bbox_points(d)
    out['angle'] = np.float64(d['pcd_rot_angle'])
    out['rot_angle_attr'] = np.float64(trk.rot_angle)
    out['rot_points'], out['rot_boxes'] = d['points'].tensor[:, :3].numpy().copy(), cat_boxes(trk)
    out['cand_rot_boxes'] = [cat_boxes(c) for c in cands]
    rst._random_scale(d)
    rst._scale_bbox_points(d)
    out['scale'] = np.float64(d['pcd_scale_factor'])
    out['scale_points'], out['scale_boxes'] = d['points'].tensor[:, :3].numpy().copy(), cat_boxes(trk)
    rst._trans_bbox_points(d)
    out['trans'] = np.asarray(d['pcd_trans'], np.float64)
    out['trans_points'], out['trans_boxes'] = d['points'].tensor[:, :3].numpy().copy(), cat_boxes(trk)
    out['cand_trans_boxes'] = [cat_boxes(c) for c in cands]
    out['mask'] = d['points'].in_range_3d(np.array(RANGE, dtype=np.float32)).numpy().copy()
    d = ref['PointsRangeFilter'](point_cloud_range=RANGE)(d)
    final = d['points'].tensor.numpy().copy()
    out['final_frame_inds'] = d['pts_frame_inds'].numpy().astype(np.int64)
    # the filtered rows are the translated coordinates, the input attributes and the frame's values under the mask: not stored
    assert np.array_equal(final[:, :3], out['trans_points'][out['mask']]) and np.array_equal(final[:, 5:], rows[of][out['mask']])
    assert np.array_equal(final[:, 3:5], np.concatenate(frames[inp['ts'].index(int(out['cut_ts'][0])):][:len(lens)], 0)[:, 3:5].astype(final.dtype)[out['mask']])
    d = ref['PointShuffle']()(d)
    shuffled = d['points'].tensor.numpy()
    assert np.array_equal(shuffled[np.lexsort(shuffled.T[::-1])], final[np.lexsort(final.T[::-1])])     # a permutation
    out['shared_pose'] = trk.shared_pose.numpy()
    return out


def run_test(ref, inp, keep=None):
    """the reference's test chain: pose, decoration (yaw, size, score), range"""
    dt = ref['dtype']
    frames = [f if keep is None else f[keep[k]] for k, f in enumerate(inp['frames'])]
    trk = build_tracklet(ref, inp['boxes'], inp['ts'], inp['scores'], inp['ts2pose'], 'p')
    d = dict(tracklet=trk, points=[torch.from_numpy(f.copy()).to(dt) for f in frames],
             pts_frame_inds=[torch.ones(len(f), dtype=torch.int) * i for i, f in enumerate(frames)])
    d = ref['TrackletPoseTransform'](concat=False)(d)
    d = ref['PointDecoration'](properties=PROPS[:3], concat=True)(d)
    out = dict(test_pose_points=d['points'].tensor[:, :3].numpy().copy(), test_boxes=cat_boxes(trk))
    center = trk.pose_list[len(trk.pose_list) // 2]
    out['test_mm'] = torch.stack([torch.linalg.inv(center) @ p for p in trk.pose_list]).numpy()
    out['test_mask'] = d['points'].in_range_3d(np.array(RANGE, dtype=np.float32)).numpy().copy()
    d = ref['PointsRangeFilter'](point_cloud_range=RANGE)(d)
    assert np.array_equal(d['points'].tensor[:, :3].numpy(), out['test_pose_points'][out['test_mask']])
    out['test_final_frame_inds'] = d['pts_frame_inds'].numpy().astype(np.int64)
    return out


def near_bound(xyz):
    r = np.array(RANGE, np.float64)
    x = np.asarray(xyz, np.float64)
    return np.any([(np.abs(x[:, k] - r[k]) < MARGIN) | (np.abs(x[:, k] - r[k + 3]) < MARGIN) for k in range(3)], 0)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if b.size else 0.0


def remove_case(ref, inp):
    """LiDARTracklet.remove of every third timestamp and one the tracklet does not have -> what is left"""
    trk = build_tracklet(ref, inp['boxes'], inp['ts'], inp['scores'], inp['ts2pose'], 'r')
    drop = (inp['ts'][::3] if len(inp['ts']) > 1 else []) + [inp['ts'][-1] + 12345]      # removing every frame cannot be frozen
    keep_idx = trk.remove(drop)
    return dict(remove_ts=np.asarray(drop, np.int64), remove_keep_idx=np.asarray(keep_idx, np.int64), remove_boxes=cat_boxes(trk),
                remove_left_ts=np.asarray(trk.ts_list, np.int64), remove_scores=np.asarray(trk.score_list, np.float64),
                remove_poses=np.stack([p.numpy() for p in trk.pose_list]),
                remove_index=np.asarray([trk.ts2index[ts] for ts in trk.ts_list], np.int64))


def draw_cases(ref):
    """three seeds, a batch of five tracklets each: what the reference's transforms draw, sample after sample"""
    out = {}
    lens = [3, 37, 160, 150, 8]
    for seed, (cons, cut) in enumerate([(False, dict(ratio=0.0, max_length=150)), (True, dict(ratio=0.5, max_cut_ratio=0.5, max_length=150)),
                                        (False, dict(ratio=0.7, max_cut_ratio=0.9, max_length=200, min_length=5))]):
        np.random.seed(seed)
        torch.manual_seed(seed)
        rows = []
        for i, n in enumerate(lens):
            log = ref['log']
            del log[:]
            ts = [T.TS0 + 100_000 * k for k in range(n)]
            boxes = np.tile(np.array([[5, 2, 0, 2, 4.5, 1.6, 0.3]], np.float32), (n, 1))
            trk = build_tracklet(ref, boxes, ts, [0.5] * n, {t: np.eye(4, dtype=np.float32) for t in ts}, 'd')
            d = dict(tracklet=trk, gt_tracklet_candidates=[], points=[torch.zeros((1, 5), dtype=ref['dtype']) for _ in range(n)],
                     pts_frame_inds=[torch.ones(1, dtype=torch.int) * k for k in range(n)])
            d = ref['TrackletCutting'](**cut)(d)
            head = int(d['pts_frame_inds'][0][0])
            tail = n - head - len(trk)
            d = ref['TrackletPoseTransform'](concat=False)(d)
            d = ref['TrackletNoise'](center_noise_cfg=dict(max_noise=NOISE['center'], consistent=cons), size_noise_cfg=None,
                                     yaw_noise_cfg=dict(max_noise=NOISE['yaw'], consistent=False))(d)
            d = ref['PointDecoration'](properties=PROPS[:3], concat=True)(d)
            d = ref['TrackletRandomFlip'](flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5)(d)
            d = ref['TrackletGlobalRotScaleTrans'](**RST)(d)
            rands = [v for k, v in log if k == 'torch.rand']
            assert len(rands) == 2
            out[f'draw{seed}_s{i}_u_center'], out[f'draw{seed}_s{i}_u_yaw'] = rands
            rows.append([head, tail, float(d['pcd_horizontal_flip']), float(d['pcd_vertical_flip']), d['pcd_rot_angle'],
                         d['pcd_scale_factor'], *np.asarray(d['pcd_trans'], np.float64), float(len([1 for k, _ in log if k != 'torch.rand']))])
        out[f'draw{seed}'] = np.array(rows, np.float64)
        out[f'draw{seed}_cfg'] = np.array([cut.get('min_length', 5), cut['ratio'], cut.get('max_cut_ratio', 0.5), cut['max_length'], float(cons)])
    out['draw_lens'] = np.asarray(lens, np.int64)
    return out


def pipeline_fixtures():
    from oracle import ref_loader
    from sst_amd.optim import resolve_config
    dst = os.path.join(ROOT, 'tests', 'golden', 'configs', 'pipeline', 'ctrl')
    os.makedirs(dst, exist_ok=True)
    for name in ('ctrl_veh_24e', 'ctrl_ped_24e', 'ctrl_cyc_12e'):
        path = os.path.join(ref_loader.REF_ROOT, 'configs', 'ctrl', name + '.py')
        cfg = resolve_config(open(path).read(), os.path.dirname(path), path)
        text = pprint.pformat({k: cfg[k] for k in ('train_pipeline', 'test_pipeline')}, width=120)
        with open(os.path.join(dst, name + '.pipeline.py'), 'w') as f:
            f.write(text + '\n')


def main():
    from oracle import ref_loader
    if not ref_loader.available():
        raise SystemExit('the reference tree is not present')
    r32, r64 = reference(False), reference(True)
    inputs = make_inputs()
    out = dict(range=np.asarray(RANGE, np.float64), n_cases=np.int64(len(CASES)))
    with M.patched(False):
        for k, case in enumerate(CASES):
            inp = inputs[case['trk']]
            first = run_train(r32, inp, case)
            # the rows of the kept frames whose final coordinates lie on the margin are taken out of the input
            head = inp['ts'].index(int(first['cut_ts'][0]))
            bad = near_bound(first['trans_points'])
            test_first = run_test(r32, inp)
            bad_test = near_bound(test_first['test_pose_points'])
            keep, at, at_test = [], 0, 0
            for f, fr in enumerate(inp['frames']):
                m = np.ones(len(fr), bool)
                m &= ~bad_test[at_test:at_test + len(fr)]
                at_test += len(fr)
                if head <= f < head + len(first['cut_ts']):
                    m &= ~bad[at:at + len(fr)]
                    at += len(fr)
                keep.append(m)
            res = run_train(r32, inp, case, keep)
            res.update(run_test(r32, inp, keep))
            assert not near_bound(res['trans_points']).any() and not near_bound(res['test_pose_points']).any()
            with M.patched(True):
                res64 = run_train(r64, inp, case, keep)
                res64.update(run_test(r64, inp, keep))
            for key in ('mm', 'pose_points', 'pose_boxes', 'noise_boxes', 'trans_points', 'trans_boxes', 'test_pose_points', 'test_mm'):
                out[f't{k}_gap_{key}'] = np.float64(rel(res[key], res64[key]))
            assert np.array_equal(res['mask'], res64['mask']) and np.array_equal(res['test_mask'], res64['test_mask'])
            if len(inp['ts']) > 10:
                assert 20 < res['mask'].sum() < len(res['mask']) - 20, (res['mask'].sum(), len(res['mask']))
            for j in range(len(inp['cands'])):
                for key in ('cand_mm', 'cand_pose_boxes', 'cand_flip_boxes', 'cand_rot_boxes', 'cand_trans_boxes'):
                    res[f'c{j}_{key[5:]}'] = res[key][j]
                res[f'c{j}_boxes'], res[f'c{j}_ts'] = inp['cands'][j]['boxes'], np.asarray(inp['cands'][j]['ts'], np.int64)
                res[f'c{j}_poses'] = np.stack([inp['ts2pose'][ts] for ts in inp['cands'][j]['ts']])
            for key in ('cand_mm', 'cand_pose_boxes', 'cand_flip_boxes', 'cand_rot_boxes', 'cand_trans_boxes'):
                del res[key]
            kept_frames = [f[m] for f, m in zip(inp['frames'], keep)]
            res.update(points=np.concatenate(kept_frames), frame_lens=np.asarray([len(f) for f in kept_frames], np.int64),
                       boxes=inp['boxes'], ts=np.asarray(inp['ts'], np.int64), scores=np.asarray(inp['scores'], np.float64),
                       poses=np.stack([inp['ts2pose'][ts] for ts in inp['ts']]), n_cands=np.int64(len(inp['cands'])),
                       flips=np.asarray(case['flips'], np.int64), consistent=np.int64(case['consistent']))
            if k < 3:
                res.update(remove_case(r32, inp))
            for key, v in res.items():
                v = np.asarray(v)
                out[f't{k}_{key}'] = v.astype(np.float32) if v.dtype == np.float64 and key not in ('angle', 'scale', 'trans', 'scores', 'cut_scores', 'remove_scores', 'rot_angle_attr') else v
            print('case', k, 'frames', len(inp['ts']), '->', len(res['cut_ts']), 'points', len(res['mask']), 'kept', int(res['mask'].sum()),
                  'test kept', int(res['test_mask'].sum()), 'of', len(res['test_mask']), {g: float(out[f't{k}_gap_{g}']) for g in ('mm', 'pose_points', 'trans_points')})
        out.update(draw_cases(r32))
    out['noise_max'] = np.asarray(NOISE['center'] + NOISE['size'] + [NOISE['yaw']], np.float64)
    out['cut_cfg'] = np.asarray([5, CUT['ratio'], 0.5, CUT['max_length']], np.float64)
    path = os.path.join(ROOT, 'tests', 'golden', 'tracklet_pipeline.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes', len(out), 'arrays')
    assert os.path.getsize(path) < 600 * 1024
    pipeline_fixtures()


if __name__ == '__main__':
    main()
