"""Generates tests/golden/cluster_head_train.npz: the training side of SparseClusterHeadV2 / FSDV2Head as the REFERENCE computes
it (data only).

Needs the reference tree (oracle.ref_loader) and its compiled points_in_boxes_cpu (oracle.build_ref); run from the
repository root:  python tests/golden/make_cluster_head_train.py

Executed from their source text: SparseClusterHeadV2.loss_single_task / get_targets / get_targets_single /
modify_gt_for_single_task / modify_gt_for_single_task_single_sample / enlarge_gt_bboxes (dense_heads/sparse_cluster_head_v2.py),
FSDV2Head.loss_single_task / get_targets / get_targets_single (fsd_v2_head.py), SparseClusterHead.split_by_batch /
combine_by_batch / assign_single / dist_constrain (sparse_cluster_head.py), BasePointBBoxCoder
(core/bbox/coders/base_point_bbox_coder.py), LiDARInstance3DBoxes.enlarged_box / points_in_boxes
(core/bbox/structures/lidar_box3d.py) and py_sigmoid_focal_loss (models/losses/focal_loss.py).  What the reference imports from
packages that are not in its tree is stood in for here:
  points_in_boxes_gpu           the reference's compiled points_in_boxes_cpu, first box per point
  mmdet FocalLoss (sigmoid)     one-hot of the labels without the background column -> py_sigmoid_focal_loss with the
                                label weights, x loss_weight
  mmdet weight_reduce_loss      (loss * weight).sum() / avg_factor, or the mean without an avg_factor
  mmdet L1Loss                  weight_reduce_loss(|pred - target|, weight, avg_factor) x loss_weight
  mmdet AssignResult,           plain records; PseudoSampler.sample: pos_inds = nonzero(gt_inds > 0), pos_assigned_gt_inds =
  PseudoSampler                 gt_inds[pos_inds] - 1, pos_gt_bboxes = gt_bboxes[pos_assigned_gt_inds]
  mmdet multi_apply             tuple(map(list, zip(*map(func, *args))))
  mmdet reduce_mean             identity (one process)
modify_gt_for_single_task_single_sample asserts that no label is negative, although get_targets_single filters such boxes
(:369-371): the scene's boxes with label -1 are taken out before the regrouping, which is what that filter would have done.
The index of the assigned box, which the reference does not return, is read from assign_single's result and mapped back through
the regrouping to the index in the concatenated boxes.  Each loss case is run in float32 and in float64; noise_* is the gap.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import cluster_head_ref as R  # noqa: E402
import seg_loss_ref as S  # noqa: E402

V2_PY = 'mmdet3d/models/dense_heads/sparse_cluster_head_v2.py'
V1_PY = 'mmdet3d/models/dense_heads/sparse_cluster_head.py'
FSDV2_PY = 'mmdet3d/models/dense_heads/fsd_v2_head.py'
CODER_PY = 'mmdet3d/core/bbox/coders/base_point_bbox_coder.py'
BOX_PY = 'mmdet3d/core/bbox/structures/lidar_box3d.py'
FOCAL_PY = 'mmdet3d/models/losses/focal_loss.py'
BATCH = 3

_CACHE = {}


class AssignResult(object):
    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels


class PseudoSampler(object):
    def sample(self, assign_result, bboxes, gt_bboxes, **kwargs):
        pos_inds = torch.nonzero(assign_result.gt_inds > 0, as_tuple=False).squeeze(-1).unique()
        neg_inds = torch.nonzero(assign_result.gt_inds == 0, as_tuple=False).squeeze(-1).unique()
        res = types.SimpleNamespace(pos_inds=pos_inds, neg_inds=neg_inds)
        res.pos_assigned_gt_inds = assign_result.gt_inds[pos_inds] - 1
        res.pos_gt_bboxes = gt_bboxes[res.pos_assigned_gt_inds] if gt_bboxes.numel() else gt_bboxes.view(-1, gt_bboxes.size(-1))
        return res


def multi_apply(func, *args):
    return tuple(map(list, zip(*map(func, *args))))


def weight_reduce_loss(loss, weight, reduction, avg_factor):
    loss = loss * weight
    return loss.mean() if avg_factor is None else loss.sum() / avg_factor


def reference_parts():
    if _CACHE:
        return _CACHE
    from oracle import build_ref, ref_loader
    build_ref.build_points_in_boxes()
    pib = build_ref.load_points_in_boxes()
    assert pib is not None, 'the reference points_in_boxes_cpu is not built'

    def points_in_boxes_gpu(points, boxes):
        pts = points[0].float().contiguous()
        bxs = boxes[0].float().contiguous()
        flags = torch.zeros((bxs.size(0), pts.size(0)), dtype=torch.int32)
        if bxs.size(0) and pts.size(0):
            pib.points_in_boxes_cpu(bxs, pts, flags)
        first = torch.where(flags.bool().any(0), flags.argmax(0), torch.full((pts.size(0),), -1)).int()
        return first[None]

    glb = dict(multi_apply=multi_apply, AssignResult=AssignResult, reduce_mean=lambda t: t)
    for name in ('loss_single_task', 'get_targets', 'get_targets_single', 'modify_gt_for_single_task',
                 'modify_gt_for_single_task_single_sample', 'enlarge_gt_bboxes'):
        _CACHE['v2.' + name] = ref_loader.load_reference_method(V2_PY, 'SparseClusterHeadV2', name, glb)
    for name in ('loss_single_task', 'get_targets', 'get_targets_single'):
        _CACHE['fsdv2.' + name] = ref_loader.load_reference_method(FSDV2_PY, 'FSDV2Head', name, glb)
    for name in ('split_by_batch', 'combine_by_batch', 'assign_single', 'dist_constrain'):
        _CACHE['v1.' + name] = ref_loader.load_reference_method(V1_PY, 'SparseClusterHead', name, glb)
    for name in ('enlarged_box', 'points_in_boxes'):
        _CACHE[name] = ref_loader.load_reference_method(BOX_PY, 'LiDARInstance3DBoxes', name,
                                                        {'points_in_boxes_gpu': points_in_boxes_gpu})
    _CACHE['coder'] = ref_loader.load_reference_class(CODER_PY, 'BasePointBBoxCoder', {'BaseBBoxCoder': object})
    _CACHE['py_sigmoid_focal_loss'] = ref_loader.load_reference_function(
        FOCAL_PY, 'py_sigmoid_focal_loss', {'F': F, 'weight_reduce_loss': weight_reduce_loss})
    return _CACHE


class Boxes(object):
    """what the heads ask of a LiDARInstance3DBoxes: indexing, cat, to, the reference's enlarged_box and points_in_boxes"""

    def __init__(self, tensor):
        self.tensor = tensor

    def __getitem__(self, item):
        return Boxes(self.tensor[item])

    def __len__(self):
        return self.tensor.size(0)

    def to(self, device):
        return self

    def new_box(self, data):
        return Boxes(data)

    def cat(self, boxes_list):
        return Boxes(torch.cat([b.tensor for b in boxes_list], 0))

    def enlarged_box(self, extra_width):
        return reference_parts()['enlarged_box'](self, extra_width)

    def points_in_boxes(self, points):
        return reference_parts()['points_in_boxes'](self, points)


def make_head(kind, tasks, class_names, code, width, train_cfg, cfg=R.LOSS_CFG):
    """a stand-in ``self`` for the reference's methods; kind: 'v2' (SparseClusterHeadV2) or 'fsdv2' (FSDV2Head)"""
    parts = reference_parts()
    head = types.SimpleNamespace()
    head.tasks, head.class_names, head.num_classes = tasks, class_names, len(class_names)
    head.bbox_coder = parts['coder'](code_size=code)
    head.box_code_size = code
    head.enlarge_width, head.train_cfg, head.training = width, train_cfg, True
    head.corner_loss_cfg = head.loss_iou = None
    head.sync_cls_avg_factor, head.sync_reg_avg_factor = False, True
    head.sampler, head.print_info = PseudoSampler(), {}
    head.assign_log = []
    for name in ('modify_gt_for_single_task', 'modify_gt_for_single_task_single_sample', 'enlarge_gt_bboxes'):
        setattr(head, name, types.MethodType(parts['v2.' + name], head))
    for name in ('loss_single_task', 'get_targets', 'get_targets_single'):
        setattr(head, name, types.MethodType(parts[kind + '.' + name], head))
    for name in ('split_by_batch', 'combine_by_batch', 'dist_constrain'):
        setattr(head, name, types.MethodType(parts['v1.' + name], head))

    def assign_single(cluster_xyz, gt_bboxes_3d, gt_labels_3d):
        res = parts['v1.assign_single'](head, cluster_xyz, gt_bboxes_3d, gt_labels_3d)
        head.assign_log.append(res.gt_inds.clone())
        return res

    head.assign_single = assign_single

    def focal(pred, label, weight, avg_factor):
        c = pred.size(1)
        target = F.one_hot(label, c + 1)[:, :c]
        return cfg['w_cls'] * parts['py_sigmoid_focal_loss'](pred, target, weight=weight, gamma=cfg['gamma'], alpha=cfg['alpha'],
                                                             reduction='mean', avg_factor=avg_factor)

    def l1(w):
        return lambda pred, target, weight, avg_factor=None: w * weight_reduce_loss((pred - target).abs(), weight, 'mean',
                                                                                     avg_factor)

    head.loss_cls = focal
    head.loss_center, head.loss_size, head.loss_rot = l1(cfg['w_center']), l1(cfg['w_size']), l1(cfg['w_rot'])
    head.loss_vel = l1(cfg['w_vel']) if code == 10 else None
    return head


def without_negative(boxes_list, labels_list):
    keep = [l >= 0 for l in labels_list]
    return [b[k] for b, k in zip(boxes_list, keep)], [l[k] for l, k in zip(labels_list, keep)], keep


def run_task(head, kind, t, logits, reg, xyz, aux, cluster_inds, boxes_list, labels_list, dtype):
    """loss_single_task of task t -> losses, gradients, the targets and the assigned boxes in the concatenated indexing"""
    fb, fl, keep = without_negative(boxes_list, labels_list)
    gt_b = [Boxes(torch.as_tensor(b).to(dtype)) for b in fb]
    gt_l = [torch.as_tensor(l) for l in fl]
    lg = torch.as_tensor(logits).to(dtype).requires_grad_(True)
    rp = torch.as_tensor(reg).to(dtype).requires_grad_(True)
    x = torch.as_tensor(xyz).to(dtype)
    inds = torch.as_tensor(cluster_inds)
    head.assign_log = []
    args = (t, lg, rp, x, inds, gt_b, gt_l)
    out = head.loss_single_task(*args, None, torch.as_tensor(aux).to(dtype)) if kind == 'fsdv2' else head.loss_single_task(*args)
    total = sum(v.reshape(-1)[0] if v.dim() else v for v in out.values())
    total.backward()
    res = {k.split('.')[0]: float(v.detach().reshape(-1)[0]) for k, v in out.items()}
    res['d_logits'] = lg.grad.numpy()
    res['d_reg'] = (rp.grad if rp.grad is not None else torch.zeros_like(rp)).numpy()
    # the targets, once more (loss_single_task does not return them), and the assigned boxes
    log = head.assign_log
    head.assign_log = []
    mod_b, mod_l = head.modify_gt_for_single_task(gt_b, gt_l, t)
    bidx = inds[:, 1]
    c = len(head.tasks[t]['class_names'])
    tgt = head.get_targets(c, x, bidx, mod_b, mod_l, rp.detach(), torch.as_tensor(aux).to(dtype)) if kind == 'fsdv2' else \
        head.get_targets(c, x, bidx, mod_b, mod_l, rp.detach())
    assert all(torch.equal(a, b) for a, b in zip(log, head.assign_log))
    labels, label_weights, bbox_targets, bbox_weights, iou_labels = tgt
    assert iou_labels is None and bool((label_weights == 1).all())
    assigned = np.full(len(xyz), -1, np.int64)
    it = iter(head.assign_log)
    base = 0
    for s in range(BATCH):
        rows = np.nonzero(cluster_inds[:, 1] == s)[0]
        orig = np.nonzero(keep[s])[0]
        perm = [orig[i] for name in head.tasks[t]['class_names'] for i in range(len(fl[s]))
                if fl[s][i] == head.class_names.index(name)]
        if len(rows):
            gt_inds = next(it).numpy()
            assert torch.equal(mod_b[s].tensor, torch.as_tensor(boxes_list[s]).to(dtype)[perm])
            pos = gt_inds > 0
            assigned[rows[pos]] = base + np.asarray(perm, np.int64)[gt_inds[pos] - 1]
        base += len(boxes_list[s])
    res.update(labels=labels.numpy(), assigned=assigned, bbox_targets=bbox_targets.numpy(), bbox_weights=bbox_weights.numpy())
    return res


# ---- the scene -----------------------------------------------------------------------------------------------------

def make_boxes(rng, n, centre, cols):
    b = np.zeros((n, cols), np.float32)
    b[:, 0:2] = centre + rng.uniform(-7, 7, (n, 2))
    b[:, 2] = rng.uniform(-1.5, -0.5, n)
    b[:, 3] = rng.uniform(1.2, 2.2, n)
    b[:, 4] = rng.uniform(2.0, 5.0, n)
    b[:, 5] = rng.uniform(1.2, 2.0, n)
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    b[1, :7] = b[0, :7] + np.float32([0.5, 0.3, 0.1, 0.2, -0.3, 0.1, 0.15])   # overlaps box 0: classes in reverse order below
    b[2, 3] = 0.3                                                           # loses its width at enlarge_width -0.2
    b[4, :7] = b[3, :7] + np.float32([-0.4, 0.5, 0.0, 0.0, 0.0, 0.0, 0.1])    # overlaps box 3 (labelled -1 below)
    b[n - 1, 0:2] = centre + np.float32([40, 40])                            # far from every row
    b[n - 2, 0:2] = centre + np.float32([-40, 43])
    if cols > 7:
        b[:, 7:9] = rng.normal(0, 2, (n, 2))
    if cols == 10:
        b[:, 9] = (np.arange(n) % 3 != 1).astype(np.float32)                 # copy-paste flags: 1, 0, 1, 1, 0 ...
    return b


def make_rows(rng, boxes_of, n):
    """n rows (sample, xyz) near the boxes of their sample, none within 1e-3 of a face at any width"""
    sample = rng.integers(0, BATCH, n)
    centres = {0: np.float32([10, 5]), 1: np.float32([0, 0]), 2: np.float32([-20, 12])}
    xyz = np.zeros((n, 3), np.float32)
    todo = np.ones(n, bool)
    every = np.concatenate([b[:, :7] for b in boxes_of if len(b)])
    while todo.any():
        for i in np.nonzero(todo)[0]:
            b = boxes_of[sample[i]]
            if len(b) and rng.random() < 0.75:
                k = rng.integers(0, len(b) - 2)
                if k == 2 and rng.random() < 0.7:    # well inside the thin box, at every width
                    xyz[i] = S.local_to_world(b[2, :7], rng.uniform(-0.35, 0.35, 1) * b[2, 4], rng.uniform(-0.2, 0.2, 1) * b[2, 3],
                                              rng.uniform(0.3, 0.7, 1))[0]
                else:
                    xyz[i] = b[k, :3] + np.float32([0, 0, 0.8]) + rng.normal(0, 1, 3).astype(np.float32) * np.float32([1.4, 1.4, 0.6])
            else:
                xyz[i, :2] = centres[sample[i]] + rng.uniform(-9, 9, 2)
                xyz[i, 2] = rng.uniform(-2, 1.5)
        todo = R.near_a_face(every, xyz)
    return sample, xyz


def f16(x):
    return x.astype(np.float16).astype(np.float32)


def main():
    rng = np.random.default_rng(20314)
    out = {}
    boxes10 = [make_boxes(rng, 9, np.float32([10, 5]), 10), np.zeros((0, 10), np.float32),
               make_boxes(rng, 8, np.float32([-20, 12]), 10)]
    # waymo labels: Cyclist (2) only on the two far boxes -> task 2 has no positive row; -1 on box 3
    labels_w = [np.array([0, 1, 0, -1, 1, 0, 1, 2, 2], np.int64), np.zeros(0, np.int64), np.array([1, 0, 1, -1, 0, 1, 2, 2], np.int64)]
    # multi labels: box 0 is a car (index 1 of task 0), box 1 a bus (index 0 of task 0): the later box comes first in the list
    labels_m = [np.array([0, 2, 4, -1, 5, 1, 3, 4, 0], np.int64), np.zeros(0, np.int64), np.array([1, 2, 5, -1, 3, 0, 4, 2], np.int64)]
    n_class = 6
    cls = np.sort(rng.integers(0, n_class, 600))                       # class-major rows: the samples interleave
    sample, xyz = make_rows(rng, boxes10, len(cls))
    cluster_inds = np.stack([cls, sample, np.arange(len(cls))], 1).astype(np.int64)
    aux = (xyz + rng.normal(0, 0.25, xyz.shape)).astype(np.float32)    # the centroids of centroid_assign
    while R.near_a_face(np.concatenate([b[:, :7] for b in boxes10 if len(b)]), aux).any():
        bad = R.near_a_face(np.concatenate([b[:, :7] for b in boxes10 if len(b)]), aux)
        aux[bad] = (xyz[bad] + rng.normal(0, 0.25, (int(bad.sum()), 3))).astype(np.float32)
    out.update(xyz=xyz, aux_xyz=aux, cluster_inds=cluster_inds)
    for s in range(BATCH):
        out[f'boxes{s}'], out[f'labels_waymo{s}'], out[f'labels_multi{s}'] = boxes10[s], labels_w[s], labels_m[s]
    n = len(xyz)
    # predictions exactly representable in float16 (stored as such); logits reach +-60 on a few rows
    logits = {'waymo': [f16(rng.normal(-1, 2, (n, 1))) for _ in range(3)],
              'multi': [f16(rng.normal(-1, 2, (n, 3))) for _ in range(2)]}
    logits['waymo'][0][:6, 0] = np.float32([60, -60, 30, -30, 60, -60])
    logits['multi'][0][:4] = np.float32([[60, -60, 0], [-60, 60, 30], [0, 0, 0], [-30, 60, -60]])
    reg = {'waymo': [f16(rng.normal(0, 1, (n, 8))) for _ in range(3)], 'multi': [f16(rng.normal(0, 1, (n, 10))) for _ in range(2)]}
    for case in logits:
        for t, (lg, rp) in enumerate(zip(logits[case], reg[case])):
            out[f'{case}_logits{t}'], out[f'{case}_reg{t}'] = lg.astype(np.float16), rp.astype(np.float16)

    # case -> (head kind, tasks, class names, box columns, labels, enlarge_width tag, train_cfg, rows)
    all_rows = np.ones(n, bool)
    cases = {}
    for tag in R.WIDTHS:
        cases[f'waymo_{tag}'] = ('v2', R.WAYMO_TASKS, R.WAYMO_NAMES, 7, labels_w, tag, {}, all_rows)
        cases[f'multi_{tag}'] = ('v2', R.MULTI_TASKS, R.MULTI_NAMES, 10, labels_m, tag, {'code_weight': R.CODE_WEIGHT10}, all_rows)
    cases['multi_centroid'] = ('fsdv2', R.MULTI_TASKS, R.MULTI_NAMES, 10, labels_m, 'p03',
                               {'code_weight': R.CODE_WEIGHT10, 'centroid_assign': True}, all_rows)
    cases['waymo_norows'] = ('v2', R.WAYMO_TASKS, R.WAYMO_NAMES, 7, labels_w, 'none', {}, sample != 2)   # sample 2 has no row
    seen = {}
    for case, (kind, tasks, names, cols, labels, tag, train_cfg, rows) in cases.items():
        code = 8 if cols == 7 else 10
        fam = case.split('_')[0]
        boxes = [b[:, :cols] for b in boxes10]
        head = make_head(kind, tasks, names, code, R.WIDTHS[tag], train_cfg)
        for t in range(len(tasks)):
            lg, rp = logits[fam][t][rows], reg[fam][t][rows]
            r32 = run_task(head, kind, t, lg, rp, xyz[rows], aux[rows], cluster_inds[rows], boxes, labels, torch.float32)
            r64 = run_task(head, kind, t, lg, rp, xyz[rows], aux[rows], cluster_inds[rows], boxes, labels, torch.float64)
            assert np.array_equal(r32['labels'], r64['labels']) and np.array_equal(r32['assigned'], r64['assigned'])
            pre = f'{case}_t{t}_'
            for k in ('labels', 'assigned', 'bbox_targets', 'bbox_weights'):
                out[pre + k] = r32[k]
            for k in r64:
                if k.startswith('loss'):
                    out[pre + 'f32_' + k], out[pre + 'f64_' + k] = np.float32(r32[k]), np.float64(r64[k])
                    out[f'noise_{pre}{k}'] = abs(r32[k] - r64[k]) / abs(r64[k]) if r64[k] else np.float64(abs(r32[k]))
                elif k.startswith('d_') and case in R.LOSS_CASES:     # the gradients of the loss cases only: size
                    out[pre + 'f64_' + k] = r64[k]
                    m = np.abs(r64[k]).max()
                    out[f'noise_{pre}{k}'] = np.abs(r32[k].astype(np.float64) - r64[k]).max() / m if m else np.float64(0)
            seen[case, t] = r32
            print(case, t, 'pos', int((r32['assigned'] >= 0).sum()), {k: r64[k] for k in r64 if k.startswith('loss')})
    # what the scene was built to contain
    assert (seen['waymo_none', 2]['assigned'] < 0).all()                                       # a task without a positive row
    for fam in ('waymo', 'multi'):
        for t in range(2):
            a = [seen[f'{fam}_{tag}', t]['assigned'] for tag in R.WIDTHS]
            assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[0], a[2])
    a = seen['multi_none', 0]['assigned']
    assert ((a == 1).sum() > 0) and (a == 0).sum() > 0                                         # box 1 (bus) wins the overlap
    hit0 = S.inside(boxes10[0][:2, :7], xyz) & (sample == 0)[None]
    both = hit0[0] & hit0[1]
    assert both.sum() >= 3 and (a[both] == 1).all()
    assert not np.array_equal(seen['multi_centroid', 0]['assigned'], seen['multi_p03', 0]['assigned'])
    w = seen['multi_none', 0]['bbox_weights']
    assert ((w[:, 8] == 0) & (w[:, 0] == 1)).any() and (w[:, 8] == 1).any()                   # flags 0 and 1 on positive rows
    thin = (seen['waymo_m02', 0]['assigned'] == 2).sum()
    assert thin > 0                                                                            # the thin box kept its extents
    path = os.path.join(ROOT, 'tests', 'golden', 'cluster_head_train.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
