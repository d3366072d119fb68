"""Writes tests/golden/augment_golden{,_s0,_s1}.npz and tests/golden/configs/pipeline/*.pipeline.py.

Runs the reference's own transform classes (ObjectSample, RandomFlip3D, GlobalRotScaleTrans, PointsRangeFilter,
ObjectRangeFilter of mmdet3d/datasets/pipelines/transforms_3d.py), box and point classes (lidar_box3d.py, base_box3d.py,
base_points.py, lidar_points.py) and box_np_ops.py from their source text, through oracle.ref_loader, under these shims:
``numba.jit`` / ``numba.njit`` are identity decorators, mmdet's ``RandomFlip`` base draws nothing and sets ``flip = False``,
``build_from_cfg`` hands ObjectSample a sampler that returns the prepared objects, the native extensions the box classes
import are empty modules.  Only data leaves: arrays in the .npz, literal dicts in the pipeline fixtures.

Runs only where the reference tree exists:  python tools/make_augment_golden.py
"""
import importlib.util
import os
import pprint
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

REF = ref_loader.REF_ROOT
RANGE = [-74.88, -74.88, -2, 74.88, 74.88, 4]
MARGIN = 1e-3


def _identity(*args, **kwargs):
    if len(args) == 1 and callable(args[0]) and not kwargs:
        return args[0]
    return lambda fn: fn


def _module(name, path=None, **attrs):
    m = types.ModuleType(name)
    if path is not None:
        m.__path__ = [path]
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    _module('numba', jit=_identity, njit=_identity)
    for name in ('mmdet3d', 'mmdet3d.ops', 'mmdet3d.core', 'mmdet3d.core.bbox'):
        _module(name, path='')
    _module('mmdet3d.ops.roiaware_pool3d', points_in_boxes_gpu=None)
    _module('mmdet3d.ops.iou3d', iou3d_cuda=None)
    pts_pkg = _module('mmdet3d.core.points', path=os.path.join(REF, 'mmdet3d/core/points'))
    base_points = _load('mmdet3d.core.points.base_points', 'mmdet3d/core/points/base_points.py')
    lidar_points = _load('mmdet3d.core.points.lidar_points', 'mmdet3d/core/points/lidar_points.py')
    pts_pkg.BasePoints = base_points.BasePoints
    _module('mmdet3d.core.bbox.structures', path=os.path.join(REF, 'mmdet3d/core/bbox/structures'))
    _load('mmdet3d.core.bbox.structures.utils', 'mmdet3d/core/bbox/structures/utils.py')
    _load('mmdet3d.core.bbox.structures.base_box3d', 'mmdet3d/core/bbox/structures/base_box3d.py')
    lidar_box = _load('mmdet3d.core.bbox.structures.lidar_box3d', 'mmdet3d/core/bbox/structures/lidar_box3d.py')
    box_np_ops = _load('mmdet3d.core.bbox.box_np_ops', 'mmdet3d/core/bbox/box_np_ops.py')

    class RandomFlip(object):                      # mmdet's base: draws nothing here, the 2-D flip is off
        def __init__(self, flip_ratio=None, **kwargs):
            self.flip_ratio = flip_ratio

        def __call__(self, results):
            results['flip'] = False
            return results

    class Sampler(object):                         # stands for DataBaseSampler: sample_all returns what the caller prepared
        def __init__(self, cfg):
            self.prepared = None

        def sample_all(self, gt_bboxes, gt_labels, img=None):
            return self.prepared

    glb = dict(np=np, box_np_ops=box_np_ops, RandomFlip=RandomFlip, build_from_cfg=lambda cfg, registry: Sampler(cfg),
               OBJECTSAMPLERS=None, LiDARInstance3DBoxes=lidar_box.LiDARInstance3DBoxes, warnings=__import__('warnings'))
    rel = 'mmdet3d/datasets/pipelines/transforms_3d.py'
    cls = {n: ref_loader.load_reference_class(rel, n, glb) for n in
           ('ObjectSample', 'RandomFlip3D', 'GlobalRotScaleTrans', 'PointsRangeFilter', 'ObjectRangeFilter')}
    for n, c in cls.items():
        glb[n] = c                                  # super(RandomFlip3D, self) looks its own name up in the globals
    return cls, lidar_box.LiDARInstance3DBoxes, lidar_points.LiDARPoints, box_np_ops


def make_scene(rng, n_points=2000, n_gt=12, n_pasted=6, cols=5):
    """one sample: points over a little more than the range, boxes inside and across the BEV bound, pasted points in their boxes"""
    def boxes(n):
        b = np.zeros((n, 7), np.float32)
        b[:, :2] = rng.uniform(-78, 78, (n, 2))
        b[:, 2] = rng.uniform(-1.5, 0.5, n)
        b[:, 3:6] = rng.uniform([1.5, 1.5, 1.2], [6.0, 3.0, 2.5], (n, 3))
        b[:, 6] = rng.uniform(-np.pi, np.pi, n)
        return b
    gt, pasted = boxes(n_gt), boxes(n_pasted)
    gt[:3, :2] = [[130, 10], [-20, -135], [-128, 128]]          # outside the BEV range under every rotation and scale drawn
    pts = np.zeros((n_points, cols), np.float32)
    pts[:, :3] = rng.uniform([-80, -80, -2.5], [80, 80, 4.5], (n_points, 3))
    # a third of the points near the pasted boxes, so that the removal has work
    near = rng.randint(0, n_pasted, n_points // 3)
    pts[:n_points // 3, :3] = pasted[near, :3] + rng.uniform(-3.5, 3.5, (n_points // 3, 3)).astype(np.float32)
    pts[:, 3:] = rng.uniform(0, 1, (n_points, cols - 3))
    own = []
    for b in pasted:
        k = 40
        local = rng.uniform(-0.45, 0.45, (k, 3)) * b[3:6]
        local[:, 2] += 0.5 * b[5]
        c, s = np.cos(b[6]), np.sin(b[6])
        xy = np.stack([local[:, 0] * c + local[:, 1] * s, -local[:, 0] * s + local[:, 1] * c], 1)
        p = np.zeros((k, cols), np.float32)
        p[:, :2], p[:, 2] = xy + b[:2], local[:, 2] + b[2]
        p[:, 3:] = rng.uniform(0, 1, (k, cols - 3))
        own.append(p)
    return dict(points=pts, gt=gt, gt_labels=rng.randint(0, 3, n_gt).astype(np.int64), pasted=pasted,
                pasted_labels=rng.randint(0, 3, n_pasted).astype(np.int64), pasted_points=np.concatenate(own))


def run_chain(ref, scene, flip_h, flip_v, seed, keep_points=None, keep_gt=None):
    """the reference classes chained in config order on one sample -> the arrays after every stage"""
    cls, Boxes, Points, _ = ref
    pts = scene['points'] if keep_points is None else scene['points'][keep_points]
    gt = scene['gt'] if keep_gt is None else scene['gt'][keep_gt]
    gt_labels = scene['gt_labels'] if keep_gt is None else scene['gt_labels'][keep_gt]
    cols = pts.shape[1]
    d = dict(points=Points(torch.from_numpy(pts.copy()), points_dim=cols), gt_bboxes_3d=Boxes(torch.from_numpy(gt.copy())),
             gt_labels_3d=gt_labels.copy(), bbox3d_fields=['gt_bboxes_3d'], box_type_3d=Boxes,
             pcd_horizontal_flip=bool(flip_h), pcd_vertical_flip=bool(flip_v))
    out = dict(in_points=pts.copy(), in_gt=gt.copy(), in_gt_labels=gt_labels.copy())
    snap = lambda: (d['points'].tensor.numpy().copy(), d['gt_bboxes_3d'].tensor.numpy().copy())

    sample = cls['ObjectSample'](db_sampler=dict(), sample_2d=False)
    sample.db_sampler.prepared = dict(gt_bboxes_3d=scene['pasted'].copy(), gt_labels_3d=scene['pasted_labels'].copy(),
                                      points=Points(torch.from_numpy(scene['pasted_points'].copy()), points_dim=cols))
    d = sample(d)
    out['s0_points'], out['s0_boxes'] = snap()
    out['s0_labels'] = d['gt_labels_3d'].copy()
    d = cls['RandomFlip3D'](sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5)(d)
    out['s1_points'], out['s1_boxes'] = snap()
    np.random.seed(seed)
    rst = cls['GlobalRotScaleTrans'](rot_range=[-0.78539816, 0.78539816], scale_ratio_range=[0.95, 1.05],
                                     translation_std=[0.2, 0.2, 0.2])
    state = np.random.get_state()
    rst._rot_bbox_points(d)
    after = np.random.get_state()
    np.random.set_state(state)                       # the angle the reference drew: its own call, replayed from the same state
    out['angle'] = np.float64(np.random.uniform(rst.rot_range[0], rst.rot_range[1]))
    np.random.set_state(after)
    out['s2_points'], out['s2_boxes'] = snap()
    rst._random_scale(d)
    rst._scale_bbox_points(d)
    out['s3_points'], out['s3_boxes'] = snap()
    rst._trans_bbox_points(d)
    out['s4_points'], out['s4_boxes'] = snap()
    out['rot_mat_T'] = d['pcd_rotation'].numpy().copy()
    out['scale'], out['trans'] = np.float64(d['pcd_scale_factor']), np.asarray(d['pcd_trans'], np.float64)
    out['point_mask'] = d['points'].in_range_3d(np.array(RANGE, dtype=np.float32)).numpy().copy()
    d = cls['PointsRangeFilter'](point_cloud_range=RANGE)(d)
    out['s5_points'] = d['points'].tensor.numpy().copy()
    orf = cls['ObjectRangeFilter'](point_cloud_range=RANGE)
    out['box_mask'] = d['gt_bboxes_3d'].in_range_bev(orf.bev_range).numpy().copy()
    d = orf(d)
    out['s5_boxes'], out['s5_labels'] = d['gt_bboxes_3d'].tensor.numpy().copy(), np.asarray(d['gt_labels_3d']).copy()
    return out


def near_bound(xyz, dims):
    r = np.array(RANGE, np.float64)
    lo, hi = r[:3], r[3:]
    x = xyz.astype(np.float64)
    return np.any([(np.abs(x[:, k] - lo[k]) < MARGIN) | (np.abs(x[:, k] - hi[k]) < MARGIN) for k in dims], 0)


def end_to_end(ref):
    """2 samples x the 4 flip combinations; inputs whose reference output lies within MARGIN of a bound are taken out"""
    out = {}
    rng = np.random.RandomState(20260101)
    scenes = [make_scene(rng), make_scene(rng)]
    for name, s in enumerate(scenes):
        for k in ('pasted', 'pasted_labels', 'pasted_points'):
            out[f'scene{name}_{k}'] = s[k]
    for fh in (0, 1):
        for fv in (0, 1):
            for si, scene in enumerate(scenes):
                seed = 100 + 10 * si + 2 * fh + fv
                first = run_chain(ref, scene, fh, fv, seed)
                n_pasted = scene['pasted_points'].shape[0]
                # s0 = [pasted rows; kept own rows]: trace the own rows back through the removal
                removed = ref[3].points_in_rbbox(scene['points'][:, :3], scene['pasted']).any(-1)
                own = np.nonzero(~removed)[0]
                bad_rows = near_bound(first['s4_points'][:, :3], (0, 1, 2))
                assert not bad_rows[:n_pasted].any(), 'a pasted point lies on the margin: change the scene'
                keep_points = np.ones(scene['points'].shape[0], bool)
                keep_points[own[bad_rows[n_pasted:]]] = False
                bad_boxes = near_bound(first['s4_boxes'][:, :3], (0, 1))
                assert not bad_boxes[scene['gt'].shape[0]:].any(), 'a pasted box lies on the margin: change the scene'
                keep_gt = ~bad_boxes[:scene['gt'].shape[0]]
                res = run_chain(ref, scene, fh, fv, seed, keep_points, keep_gt)
                assert not near_bound(res['s4_points'][:, :3], (0, 1, 2)).any()
                assert not near_bound(res['s4_boxes'][:, :3], (0, 1)).any()
                assert res['point_mask'].sum() > 100 and (~res['point_mask']).sum() > 10
                assert res['box_mask'].sum() > 3 and (~res['box_mask']).sum() > 0, (res['box_mask'])
                assert res['s0_points'].shape[0] < n_pasted + res['in_points'].shape[0] - 10     # the removal had work
                # what the arrays below leave out is implied by what they keep: checked here, once
                kept_own = ~ref[3].points_in_rbbox(res['in_points'][:, :3], scene['pasted']).any(-1)
                assert np.array_equal(res['s0_points'], np.concatenate([scene['pasted_points'], res['in_points'][kept_own]]))
                assert np.array_equal(res['s0_boxes'], np.concatenate([res['in_gt'], scene['pasted']]))
                assert np.array_equal(res['s5_points'], res['s4_points'][res['point_mask']])
                for st in ('s1', 's2', 's3', 's4'):
                    assert np.array_equal(res[st + '_points'][:, 3:], res['s0_points'][:, 3:])
                    res[st + '_points'] = res[st + '_points'][:, :3].copy()
                res['kept_own'], res['keep_points'], res['keep_gt'] = kept_own, keep_points, keep_gt
                for k in ('s0_points', 's0_boxes', 's5_points', 'in_points', 'in_gt', 'in_gt_labels'):
                    del res[k]
                for k, v in res.items():
                    out[f'e2e_h{fh}v{fv}_smp{si}_{k}'] = v
    for name, s in enumerate(scenes):
        for k in ('points', 'gt', 'gt_labels'):
            out[f'scene{name}_{k}'] = s[k]
    return out


def points_in_boxes_cases(ref):
    _, _, _, ops = ref
    rng = np.random.RandomState(7)
    n, m = 12, 1500
    boxes = np.zeros((n, 7), np.float32)
    boxes[:, :3] = rng.uniform(-20, 20, (n, 3))
    boxes[:, 3:6] = rng.uniform(0.5, 6, (n, 3))
    boxes[:, 6] = rng.uniform(-4, 4, n)
    pts = (boxes[rng.randint(0, n, m), :3] + rng.uniform(-4, 4, (m, 3))).astype(np.float32)
    corners = ops.center_to_corner_box3d(boxes[:, :3], boxes[:, 3:6], boxes[:, 6], origin=(0.5, 0.5, 0), axis=2)
    normal, d = ops.surface_equ_3d(ops.corner_to_surfaces_3d(corners))
    sgn = (pts[:, None, None, 0] * normal[None, ..., 0] + pts[:, None, None, 1] * normal[None, ..., 1]
           + pts[:, None, None, 2] * normal[None, ..., 2] + d[None])
    pts = pts[(np.abs(sgn) >= 1e-4).all((1, 2))]
    assert pts.shape[0] > 1000 and pts.dtype == np.float32
    mask = ops.points_in_rbbox(pts, boxes)
    assert mask.any() and not mask.all()
    out = dict(pib_boxes=boxes, pib_points=pts, pib_mask=mask, pib_normal=normal.astype(np.float32), pib_d=d.astype(np.float32))
    # dyadic axis-aligned boxes: every product and sum is exact on both sides; points on faces, edges and corners
    dy = np.array([[0, 0, 0, 2, 4, 2, 0], [8, -4, 1, 1, 0.5, 4, 0], [-16, 2, -1, 8, 2, 1, 0]], np.float32)
    grid = []
    for b in dy:
        xs = [b[0] - b[3] / 2, b[0] - b[3] / 4, b[0], b[0] + b[3] / 2, b[0] + b[3]]
        ys = [b[1] - b[4] / 2, b[1], b[1] + b[4] / 4, b[1] + b[4] / 2, b[1] - b[4]]
        zs = [b[2], b[2] + b[5] / 2, b[2] + b[5], b[2] - b[5] / 4, b[2] + b[5] / 4]
        grid += [(x, y, z) for x in xs for y in ys for z in zs]
    dpts = np.array(grid, np.float32)
    dmask = ops.points_in_rbbox(dpts, dy)
    assert dmask.any()
    out.update(dyadic_boxes=dy, dyadic_points=dpts, dyadic_mask=dmask)
    return out


def draw_cases(ref):
    """3 seeds, a batch of 2: the reference's transforms consume np.random sample after sample"""
    cls, Boxes, Points, _ = ref
    out = {}
    for seed in (0, 1, 2):
        np.random.seed(seed)
        rows = []
        for _ in range(2):
            box = torch.tensor([[10.0, 5.0, 0.0, 4.0, 2.0, 1.5, 0.0]])
            d = dict(points=Points(torch.tensor([[1.0, 2.0, 0.5]]), points_dim=3), gt_bboxes_3d=Boxes(box),
                     bbox3d_fields=['gt_bboxes_3d'], box_type_3d=Boxes)
            d = cls['RandomFlip3D'](sync_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5)(d)
            state = np.random.get_state()
            angle = np.float64(np.random.uniform(-0.78539816, 0.78539816))     # the first draw of the call below, replayed
            np.random.set_state(state)
            d = cls['GlobalRotScaleTrans'](rot_range=[-0.78539816, 0.78539816], scale_ratio_range=[0.95, 1.05],
                                           translation_std=[0.5, 0.5, 0.2])(d)
            rot = d['pcd_rotation'].numpy()
            rows.append([float(d['pcd_horizontal_flip']), float(d['pcd_vertical_flip']), rot[0, 0], rot[1, 0],
                         d['pcd_scale_factor'], *np.asarray(d['pcd_trans'], np.float64),
                         np.float64(np.float32(angle))])
            assert rot[0, 0] == np.cos(np.float32(angle)) or abs(rot[0, 0] - np.cos(angle)) < 1e-6
        out[f'draw_seed{seed}'] = np.array(rows, np.float64)
    return out


def pipeline_fixtures():
    from sst_amd.optim import resolve_config
    dst = os.path.join(ROOT, 'tests', 'golden', 'configs', 'pipeline')
    os.makedirs(dst, exist_ok=True)
    names = ('sst/sst_waymoD5_1x_3class_8heads_3f', 'sst_refactor/sst_waymoD5_1x_3class_8heads_v2',
             'sst_refactor/sst_waymoD5_1x_3class_centerhead', 'fsd/fsd_waymoD1_1x', 'fsd/fsd_waymoD1_1x_3f',
             'fsdv2/fsdv2_waymo_1x', 'fsdv2/fsdv2_nusc_1x', 'fsdv2/fsdv2_argo_2x', 'fsdpp/fsdpp_waymoD1_1x_7f_6base')
    for name in names:
        path = os.path.join(REF, 'configs', name + '.py')
        if not os.path.exists(path):
            print('no such config:', name)
            continue
        cfg = resolve_config(open(path).read(), os.path.dirname(path), path)
        text = pprint.pformat({k: cfg[k] for k in ('train_pipeline', 'test_pipeline')}, width=120)
        with open(os.path.join(dst, os.path.basename(name) + '.pipeline.py'), 'w') as f:
            f.write(text + '\n')


def main():
    if not ref_loader.available():
        raise SystemExit('the reference tree is not present')
    ref = load_reference()
    e2e = end_to_end(ref)
    small = dict(points_in_boxes_cases(ref))
    small.update(draw_cases(ref))
    # one file per sample of the end-to-end case (each stays under the size limit of a committed file), one for the rest
    files = {'augment_golden_s0.npz': {k: v for k, v in e2e.items() if '_smp0_' in k or k.startswith('scene0_')},
             'augment_golden_s1.npz': {k: v for k, v in e2e.items() if '_smp1_' in k or k.startswith('scene1_')},
             'augment_golden.npz': small}
    assert sum(len(f) for f in files.values()) == len(e2e) + len(small)
    for name, arrays in files.items():
        path = os.path.join(ROOT, 'tests', 'golden', name)
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path), 'bytes,', len(arrays), 'arrays')
        assert os.path.getsize(path) < 1 << 20
    pipeline_fixtures()


if __name__ == '__main__':
    main()
