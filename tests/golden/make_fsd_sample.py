"""Generates tests/golden/fsd_sample.npz: the FSD foreground sampling stage as the REFERENCE computes it (data only).

Needs the reference tree (oracle.ref_loader) and its compiled points_in_boxes_cpu (oracle.build_ref); run from the repository
root:  python tests/golden/make_fsd_sample.py

Executed from their source text on the CPU: SingleStageFSD.sample / get_fg_mask / get_sample_beg_position / split_by_batch /
combine_by_batch / update_sample_results_by_mask / combine_classes / pre_voxelize (detectors/single_stage_fsd.py),
FSD.prepare_multi_class_roi_input / prepare_roi_input (detectors/two_stage_fsd.py) and LiDARInstance3DBoxes.points_in_boxes
(core/bbox/structures/lidar_box3d.py).  What these import from outside the tree or from compiled extensions is stood in for:
  get_inner_win_inds     oracle.ref_loader.stable_ingroup_rank (rank of every element inside its group, stable)
  scatter_v2 ('avg')     the mean of the rows of every group of the given inverse map (index_add / counts), -> (means, new_coors)
  points_in_boxes_gpu    the reference's compiled points_in_boxes_cpu, first box per point
  Tensor.sort()          of prepare_multi_class_roi_input (two_stage_fsd.py:174): the STABLE sort.  The reference does not ask for
                         stability, so its order inside a sample is whatever the sort of the day gives (torch's CPU sort moves
                         equal keys); the library fixes the stable order, and that is what is recorded.  The
                         batch indices go in as a tensor subclass whose ``sort`` is ``torch.sort(stable=True)``.
The detector object is a plain record with the attributes the methods read (cfg / train_cfg / test_cfg, training, runtime_info,
num_classes, cluster_assigner.point_cloud_range).  The cluster filter between sample and update_sample_results_by_mask is a
drawn valid mask per class (the assigners have goldens of their own).  Feature and vote-prediction values are small integers and
the points multiples of 1/64 (they are only copied; the file compresses); the vote offsets and the logits are real.  Every logit's float64 sigmoid is at least 1e-6 away from the
float32 threshold of its class.  center_preds is also run in float64; pre_voxelize passes float32 / float16 tensors only, so its
float64 means are the stand-in's over the same groups (``*_f64``)."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import fsd_sample_ref as R  # noqa: E402

SS_PY = 'mmdet3d/models/detectors/single_stage_fsd.py'
TS_PY = 'mmdet3d/models/detectors/two_stage_fsd.py'
BOX_PY = 'mmdet3d/core/bbox/structures/lidar_box3d.py'
KEYS = ('seg_points', 'seg_logits', 'seg_vote_preds', 'seg_feats', 'batch_idx', 'vote_offsets')


class Cfg(dict):
    __getattr__ = dict.get


def scatter_avg(feat, coors, mode, return_inv=True, min_points=0, unq_inv=None, new_coors=None):
    assert mode == 'avg' and unq_inv is not None and new_coors is not None and min_points == 0
    out = torch.zeros((new_coors.size(0), feat.size(1)), dtype=feat.dtype).index_add_(0, unq_inv, feat)
    cnt = torch.zeros(new_coors.size(0), dtype=feat.dtype).index_add_(0, unq_inv, torch.ones(feat.size(0), dtype=feat.dtype))
    return out / cnt[:, None], new_coors


def reference_parts():
    from oracle import build_ref, ref_loader
    build_ref.build_points_in_boxes()
    pib = build_ref.load_points_in_boxes()
    assert pib is not None, 'the reference points_in_boxes_cpu is not built'

    def points_in_boxes_gpu(points, boxes):
        pts, bxs = points[0].float().contiguous(), boxes[0].float().contiguous()
        flags = torch.zeros((bxs.size(0), pts.size(0)), dtype=torch.int32)
        if bxs.size(0) and pts.size(0):
            pib.points_in_boxes_cpu(bxs, pts, flags)
        return torch.where(flags.bool().any(0), flags.argmax(0), torch.full((pts.size(0),), -1)).int()[None]

    glb = {'get_inner_win_inds': ref_loader.stable_ingroup_rank, 'scatter_v2': scatter_avg}
    parts = {name: ref_loader.load_reference_method(SS_PY, 'SingleStageFSD', name, glb)
             for name in ('sample', 'get_fg_mask', 'get_sample_beg_position', 'split_by_batch', 'combine_by_batch',
                          'update_sample_results_by_mask', 'combine_classes', 'pre_voxelize')}
    for name in ('prepare_multi_class_roi_input', 'prepare_roi_input'):
        parts[name] = ref_loader.load_reference_method(TS_PY, 'FSD', name)
    parts['points_in_boxes'] = ref_loader.load_reference_method(BOX_PY, 'LiDARInstance3DBoxes', 'points_in_boxes',
                                                                {'points_in_boxes_gpu': points_in_boxes_gpu})
    return parts


class StableSort(torch.Tensor):
    def sort(self, *args, **kwargs):
        return torch.sort(self.as_subclass(torch.Tensor), stable=True)


class Boxes(object):
    def __init__(self, tensor, parts):
        self.tensor, self.parts = tensor, parts

    def __getitem__(self, item):
        return Boxes(self.tensor[item], self.parts)

    def __len__(self):
        return self.tensor.size(0)

    def points_in_boxes(self, points):
        return self.parts['points_in_boxes'](self, points)


def detector(parts, num_classes, cfg, training, runtime_info=None):
    det = types.SimpleNamespace(num_classes=num_classes, cfg=cfg, train_cfg=cfg, test_cfg=cfg, training=training,
                                runtime_info=runtime_info if runtime_info is not None else {},
                                cluster_assigner=types.SimpleNamespace(point_cloud_range=[-40., -40., -4., 40., 40., 4.]))
    for name, fn in parts.items():
        if name != 'points_in_boxes':
            setattr(det, name, types.MethodType(fn, det))
    return det


def run_case(out, parts, name, data, cfg, training=False, runtime_info=None, gts=None, seed=0):
    c = data['seg_logits'].size(1)
    batch = int(data['batch_idx'].max()) + 1
    det = detector(parts, c, Cfg(cfg), training, runtime_info)
    topk = training and cfg.get('disable_pretrain', False) and not (runtime_info or {}).get('enable_detection', False)
    buf = (runtime_info or {}).get('threshold_buffer', 0) if training else 0
    thr = [float('inf')] * c if topk else R.thresholds32(cfg['score_thresh'], buf)
    assert bool(R.margin_ok(data['seg_logits'], thr).all()), name
    boxes = labels = None
    if gts is not None:
        boxes, labels = [Boxes(b, parts) for b in gts[0]], gts[1]
    scores, xyz = data['seg_logits'].sigmoid(), data['seg_points'][:, :3]
    pre = [det.get_fg_mask(scores, xyz, k, data['batch_idx'], boxes, labels) for k in range(c)]
    rule = [len(torch.unique(data['batch_idx'][m])) < batch for m in pre]
    extra = None
    if topk:
        extra = torch.stack(pre)
    elif gts is not None:                # the ground-truth part alone: thresholds no score reaches
        only = detector(parts, c, Cfg(dict(cfg, score_thresh=[2.0] * c)), training, runtime_info)
        extra = torch.stack([only.get_fg_mask(scores, xyz, k, data['batch_idx'], boxes, labels) for k in range(c)])
    smp = det.sample(dict(data), data['vote_offsets'], boxes, labels)
    d64 = {k: (v.double() if v.is_floating_point() and k != 'seg_logits' else v) for k, v in data.items()}
    smp64 = det.sample(dict(d64), d64['vote_offsets'], boxes, labels)
    for k in KEYS:
        out[f'{name}_{k}'] = data[k].numpy()
    out[f'{name}_thr32'] = np.array(thr, dtype=np.float64)
    out[f'{name}_batch'] = np.int64(batch)
    out[f'{name}_rule'] = np.array(rule)
    if extra is not None:
        out[f'{name}_extra'] = extra.numpy()
    g = torch.Generator().manual_seed(seed)
    valid = [torch.rand(m.size(0), generator=g) < 0.75 for m in smp['seg_points']]
    for k in range(c):
        for key in ('seg_points', 'batch_idx', 'center_preds'):
            out[f'{name}_s_{key}_{k}'] = smp[key][k].numpy()
        if name == 'plain':
            out[f'{name}_s_center_preds_f64_{k}'] = smp64['center_preds'][k].numpy()
        out[f'{name}_s_fg_mask_{k}'] = smp['fg_mask_list'][k].numpy()
        out[f'{name}_valid_{k}'] = valid[k].numpy()
    upd = det.update_sample_results_by_mask(dict(smp), valid)
    comb = det.combine_classes(upd, ['seg_points', 'seg_logits', 'seg_vote_preds', 'seg_feats', 'center_preds'])
    pts_feats = torch.cat([comb['seg_logits'], comb['seg_vote_preds'], comb['seg_feats']], dim=1)
    out[f'{name}_pts_feats'] = pts_feats.numpy()
    out[f'{name}_points'] = comb['seg_points'].numpy()
    out[f'{name}_center_preds'] = comb['center_preds'].numpy()
    for k in range(c):
        out[f'{name}_final_mask_{k}'] = upd['fg_mask_list'][k].numpy()
    cluster = torch.randint(-1, 2, (pts_feats.size(0), 5), generator=g).float()
    out[f'{name}_cluster_pts_feats'] = cluster.numpy()
    prepare = det.prepare_roi_input if c == 1 else det.prepare_multi_class_roi_input
    pts, feats, bidx = prepare(data['seg_points'], cluster, data['seg_feats'], upd['fg_mask_list'],
                               data['batch_idx'].as_subclass(StableSort), comb['seg_points'])
    pts, feats, bidx = (t.as_subclass(torch.Tensor) for t in (pts, feats, bidx))
    out[f'{name}_roi_points'], out[f'{name}_roi_feats'], out[f'{name}_roi_batch'] = pts.numpy(), feats.numpy(), bidx.numpy()
    print(f'{name}: N {data["seg_points"].size(0)}, selected {[int(m.sum()) for m in smp["fg_mask_list"]]}, rule {rule}, '
          f'kept {pts_feats.size(0)}, RoI rows {pts.size(0)}')


def case_data(n, c, b, seed, thr, fg=0.3):
    data, _ = R.make_case(n, c, b, 67, seed=seed, fg=fg, int_feats=True)
    data['seg_feats'] = data['seg_feats'].clamp(-1, 1)
    data['seg_points'] = torch.round(data['seg_points'] * 64) / 64      # copied rows: short mantissas compress; the centre add still rounds
    data['seg_logits'] = R.redraw_until_clear(data['seg_logits'], thr, torch.Generator().manual_seed(seed + 2))
    return data


def main():
    parts = reference_parts()
    out, names = {}, []

    def add(name, *a, **kw):
        names.append(name)
        run_case(out, parts, name, *a, **kw)

    base = dict(score_thresh=[0.5, 0.3, 0.6])
    thr = R.thresholds32(base['score_thresh'])
    add('plain', case_data(400, 3, 2, 1, thr), base, seed=1)

    data = case_data(300, 3, 3, 2, thr, fg=0.4)            # class 0 empty in sample 1; the first point of sample 0 selected
    first = [int(torch.nonzero(data['batch_idx'] == s)[0, 0]) for s in range(3)]
    data['seg_logits'][data['batch_idx'] == 1, 0] = -3.0
    data['seg_logits'][first[0], 0], data['seg_logits'][first[2], 0] = 3.0, -3.0
    add('rule_pair', data, base, seed=2)

    info = dict(threshold_buffer=0.1, enable_detection=True)
    thr_b = R.thresholds32(base['score_thresh'], 0.1)
    add('buffer', case_data(300, 3, 2, 3, thr_b), base, training=True, runtime_info=info, seed=3)

    data = case_data(300, 3, 2, 4, [float('inf')] * 3)
    for k in range(3):                                     # pairwise distinct scores per class
        data['seg_logits'][:, k] = torch.linspace(-3, 3, 300)[torch.randperm(300, generator=torch.Generator().manual_seed(k))]
    add('topk', data, dict(base, disable_pretrain=True, disable_pretrain_topks=[40, 20, 400]), training=True, runtime_info={}, seed=4)

    data = case_data(300, 3, 2, 5, thr, fg=0.15)
    g = torch.Generator().manual_seed(55)
    boxes, labels = [], []
    for s in range(2):
        rows = torch.nonzero(data['batch_idx'] == s)[:, 0]
        ctr = data['seg_points'][rows[torch.randperm(rows.numel(), generator=g)[:5]], :3]
        boxes.append(torch.cat([ctr[:, :2], ctr[:, 2:3] - 3., torch.full((5, 3), 8.), torch.rand(5, 1, generator=g)], 1))
        labels.append(torch.tensor([0, 1, 2, 0, 1]))
    add('gt_points', data, dict(base, add_gt_fg_points=True), gts=(boxes, labels), seed=5)
    out['gt_points_gt_boxes'] = torch.stack(boxes).numpy()
    out['gt_points_gt_labels'] = torch.stack(labels).numpy()

    data = case_data(300, 3, 2, 6, thr)
    data['seg_logits'][:, 1] = -6.0                        # a class that selects nothing before the rule
    add('class_none', data, base, seed=6)

    data = case_data(300, 3, 3, 7, thr)
    data['seg_logits'][:, 2] = 6.0                         # a class that selects everything
    add('class_all', data, base, seed=7)

    add('single', case_data(350, 1, 2, 8, R.thresholds32([0.4])), dict(score_thresh=[0.4]), seed=8)
    out['cases'] = np.array(names)

    # pre_voxelize: a small cloud, 0.5 m voxels; float32 and float64
    g = torch.Generator().manual_seed(9)
    n = 240
    pv = dict(seg_points=torch.cat([torch.rand(n, 3, generator=g) * torch.tensor([6., 6., 2.]) - torch.tensor([3., 3., 1.]),
                                    torch.rand(n, 1, generator=g)], 1),
              seg_logits=torch.randn(n, 3, generator=g), seg_vote_preds=torch.randn(n, 9, generator=g),
              seg_feats=torch.randn(n, 8, generator=g), batch_idx=torch.sort(torch.randint(0, 2, (n,), generator=g))[0],
              vote_offsets=torch.randn(n, 9, generator=g))
    det = detector(parts, 3, Cfg(dict(base, pre_voxelization_size=(0.5, 0.5, 0.5))), False)
    res32 = det.pre_voxelize(dict(pv))
    lo = torch.tensor(det.cluster_assigner.point_cloud_range[:3])
    coors = torch.div(pv['seg_points'][:, :3] - lo[None], torch.tensor([0.5, 0.5, 0.5])[None], rounding_mode='floor').long()
    coors = torch.cat([pv['batch_idx'][:, None], coors[:, [2, 1, 0]]], 1)
    new_coors, inv = torch.unique(coors, return_inverse=True, dim=0)
    out['pv_new_coors'], out['pv_unq_inv'] = new_coors.numpy(), inv.numpy()
    out['pv_pc_range'] = np.array(det.cluster_assigner.point_cloud_range)
    for k in KEYS:
        out[f'pv_in_{k}'] = pv[k].numpy()
        out[f'pv_out_{k}'] = res32[k].numpy()
        if k in ('seg_points', 'seg_feats'):   # pre_voxelize passes float32 / float16 tensors only (:610): the float64 means over the same groups
            out[f'pv_out_f64_{k}'] = scatter_avg(pv[k].double(), coors, 'avg', unq_inv=inv, new_coors=new_coors)[0].numpy()
    print(f'pre_voxelize: {n} points -> {new_coors.size(0)} voxels')

    # column-major storage of the matrices (np.load gives the same values back): columns of one kind compress far better than rows
    out = {k: np.asfortranarray(v) if isinstance(v, np.ndarray) and v.ndim == 2 else v for k, v in out.items()}
    path = os.path.join(ROOT, 'tests', 'golden', 'fsd_sample.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays')


if __name__ == '__main__':
    main()
