"""Generates tests/golden/seg_head_train.npz: VoteSegHead's training side as the REFERENCE computes it (data only).

Needs the reference tree (oracle.ref_loader) and its compiled points_in_boxes_cpu (oracle.build_ref); run from the
repository root:  python tests/golden/make_seg_head_train.py

The reference's own VoteSegHead.get_targets / get_point_labels / get_vote_target / encode_vote_targets / losses /
gather_group_by_names (decode_heads/segmentation_head.py), LiDARInstance3DBoxes.enlarged_box_hw / gravity_center /
points_in_boxes (core/bbox/structures/lidar_box3d.py) and py_sigmoid_focal_loss (models/losses/focal_loss.py) are executed
from their source text.  What the reference imports from packages that are not in its tree is stood in for here:
  points_in_boxes_gpu           the reference's compiled points_in_boxes_cpu, first box per point
  mmdet FocalLoss (sigmoid)     one-hot of the labels without the background column -> py_sigmoid_focal_loss, mean, x weight
  mmseg weight_reduce_loss      (loss * weight).mean()
  mmseg CrossEntropyLoss        F.cross_entropy(reduction='none', weight=class_weight).mean() x loss_weight
  mmdet L1Loss                  |pred - target|.mean() x loss_weight
Each loss case is run in float32 and in float64; noise_* is the gap between the two runs.
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

import seg_loss_ref as R  # noqa: E402

HEAD_PY = 'mmdet3d/models/decode_heads/segmentation_head.py'
BOX_PY = 'mmdet3d/core/bbox/structures/lidar_box3d.py'
FOCAL_PY = 'mmdet3d/models/losses/focal_loss.py'
WIDTHS = {'none': None, 'p02': 0.2, 'm03': -0.3}
WAYMO_NAMES, WAYMO_THRESH = ('Car', 'Ped', 'Cyc'), (0.3, 0.25, 0.25)

_CACHE = {}


def reference_parts():
    """the reference's methods as plain functions + the compiled membership routine"""
    if _CACHE:
        return _CACHE
    from oracle import build_ref, ref_loader
    build_ref.build_points_in_boxes()
    pib = build_ref.load_points_in_boxes()
    assert pib is not None, 'the reference points_in_boxes_cpu is not built'

    def points_in_boxes_gpu(points, boxes):
        """[1, P, 3], [1, G, 7] -> [1, P]: first box holding the point, -1 for none (points_in_boxes.py:6-47)"""
        pts = points[0].float().contiguous()
        bxs = boxes[0].float().contiguous()
        flags = torch.zeros((bxs.size(0), pts.size(0)), dtype=torch.int32)
        if bxs.size(0) and pts.size(0):
            pib.points_in_boxes_cpu(bxs, pts, flags)
        first = torch.where(flags.bool().any(0), flags.argmax(0), torch.full((pts.size(0),), -1)).int()
        return first[None]

    for name in ('get_targets', 'get_point_labels', 'get_vote_target', 'encode_vote_targets', 'losses',
                 'gather_group_by_names'):
        _CACHE[name] = ref_loader.load_reference_method(HEAD_PY, 'VoteSegHead', name)
    for name in ('enlarged_box_hw', 'gravity_center', 'points_in_boxes'):
        _CACHE[name] = ref_loader.load_reference_method(BOX_PY, 'LiDARInstance3DBoxes', name,
                                                        {'points_in_boxes_gpu': points_in_boxes_gpu})
    _CACHE['py_sigmoid_focal_loss'] = ref_loader.load_reference_function(
        FOCAL_PY, 'py_sigmoid_focal_loss',
        {'F': F, 'weight_reduce_loss': lambda loss, weight, reduction, avg_factor: (loss * weight).mean()})
    return _CACHE


class Boxes(object):
    """what get_targets asks of a LiDARInstance3DBoxes: indexing by a mask, the reference's enlarged_box_hw, gravity_center
    and points_in_boxes"""

    def __init__(self, tensor):
        self.tensor = tensor

    device = property(lambda self: self.tensor.device)
    bottom_center = property(lambda self: self.tensor[:, :3])
    gravity_center = property(lambda self: reference_parts()['gravity_center'](self))

    def __getitem__(self, item):
        return Boxes(self.tensor[item])

    def __len__(self):
        return self.tensor.size(0)

    def new_box(self, data):
        return Boxes(data)

    def enlarged_box_hw(self, extra_width):
        return reference_parts()['enlarged_box_hw'](self, extra_width)

    def points_in_boxes(self, points):
        return reference_parts()['points_in_boxes'](self, points)


def make_head(use_sigmoid, num_classes, train_cfg, logit_scale=1.0, gamma=3.0, alpha=0.8, class_weight=None,
              w_decode=1.0, w_vote=1.0):
    """a stand-in ``self`` for the reference's methods"""
    parts = reference_parts()
    head = types.SimpleNamespace()
    head.use_sigmoid, head.bg_label = use_sigmoid, num_classes
    head.num_classes = num_classes if use_sigmoid else num_classes + 1
    head.logit_scale, head.train_cfg, head.loss_aux = logit_scale, train_cfg, None
    for name in ('get_targets', 'get_point_labels', 'get_vote_target', 'encode_vote_targets', 'losses',
                 'gather_group_by_names'):
        setattr(head, name, types.MethodType(parts[name], head))

    def focal(pred, label):
        target = F.one_hot(label, num_classes + 1)[:, :num_classes]
        return w_decode * parts['py_sigmoid_focal_loss'](pred, target, gamma=gamma, alpha=alpha)

    def cross_entropy(pred, label):
        w = None if class_weight is None else pred.new_tensor(class_weight)
        return w_decode * F.cross_entropy(pred, label, weight=w, reduction='none').mean()

    head.loss_decode = focal if use_sigmoid else cross_entropy
    head.loss_vote = lambda pred, target: w_vote * (pred - target).abs().mean()
    return head


def reference_targets(head, points_list, boxes_list, labels_list):
    """the reference's get_targets on numpy inputs -> (labels, vote_targets, vote_mask) as numpy"""
    labels, targets, mask = head.get_targets([torch.as_tensor(p) for p in points_list],
                                             [Boxes(torch.as_tensor(b)) for b in boxes_list],
                                             [torch.as_tensor(l) for l in labels_list])
    return labels.numpy(), targets.numpy(), mask.numpy()


def reference_losses(head, logits, vote_preds, labels, targets, mask, dtype):
    lg = torch.as_tensor(logits).to(dtype).requires_grad_(True)
    vp = torch.as_tensor(vote_preds).to(dtype).requires_grad_(True)
    out = head.losses(lg, vp, torch.as_tensor(labels), torch.as_tensor(targets).to(dtype), torch.as_tensor(mask))
    out['loss_sem_seg'].backward()
    if out['loss_vote'].requires_grad:
        out['loss_vote'].backward()
    res = {k: np.asarray(v.detach().reshape(-1).numpy()) for k, v in out.items()}
    res['d_logits'] = lg.grad.numpy()
    res['d_vote_preds'] = (vp.grad if vp.grad is not None else torch.zeros_like(vp)).numpy()
    return res


# ---- the scene -----------------------------------------------------------------------------------------------------

def make_boxes(rng, n, centre):
    b = np.zeros((n, 7), np.float32)
    b[:, 0:2] = centre + rng.uniform(-6, 6, (n, 2))
    b[:, 2] = rng.uniform(-1.5, -0.5, n)
    b[:, 3] = rng.uniform(1.2, 2.2, n)
    b[:, 4] = rng.uniform(2.0, 5.0, n)
    b[:, 5] = rng.uniform(1.2, 2.0, n)
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    b[1, :] = b[0, :] + np.float32([0.6, 0.3, 0.1, 0.2, -0.3, 0.1, 0.2])     # overlaps box 0
    b[2, 3] = 0.5                                                         # loses its width at extra_width -0.3
    b[4, :] = b[3, :] + np.float32([-0.4, 0.5, 0.0, 0.0, 0.0, 0.0, 0.1])      # overlaps box 3 (labelled -1 below)
    return b


def make_points(rng, boxes, n):
    pts = np.zeros((n, 4), np.float32)
    todo = np.ones(n, bool)
    while todo.any():
        k = int(todo.sum())
        which = rng.integers(0, len(boxes), k)
        near = boxes[which, :3] + np.float32([0, 0, 0.8]) + rng.normal(0, 1, (k, 3)).astype(np.float32) * np.float32([1.6, 1.6, 0.6])
        far = boxes[:, :3].mean(0) + rng.uniform(-12, 12, (k, 3)).astype(np.float32) * np.float32([1, 1, 0.2])
        cand = np.where(rng.random((k, 1)) < 0.7, near, far)
        # the first points lie well inside the 0.5 m wide box 2, which keeps them at every extra width
        pin = R.local_to_world(boxes[2], rng.uniform(-0.4, 0.4, k) * boxes[2, 4], rng.uniform(-0.3, 0.3, k) * boxes[2, 3],
                               rng.uniform(0.2, 0.8, k))
        pts[todo, :3] = np.where((np.nonzero(todo)[0] < 12)[:, None], pin, cand)
        todo = R.near_a_face(boxes, pts[:, :3], [w for w in WIDTHS.values() if w is not None])
    pts[:, 3] = rng.random(n)
    return pts


def away_from_thresholds(rng, make, margin_of, tol=1e-4):
    x = make(rng)
    while True:
        bad = margin_of(x) < tol
        if not bad.any():
            return x
        x[bad] = make(rng)[bad]


def main():
    rng = np.random.default_rng(20260)
    out = {}
    boxes = [make_boxes(rng, 7, np.float32([10, 5])), make_boxes(rng, 6, np.float32([-20, 12]))]
    points = [make_points(rng, boxes[0], 300), make_points(rng, boxes[1], 280)]
    labels3 = [np.array([0, 1, 2, -1, 0, 2, 1], np.int64), np.array([2, 0, 1, -1, 1, 0], np.int64)]
    labels10 = [np.array([0, 7, 4, -1, 9, 5, 2], np.int64), np.array([8, 1, 3, -1, 6, 0], np.int64)]
    for s in range(2):
        out[f'points{s}'], out[f'boxes{s}'], out[f'labels3_{s}'], out[f'labels10_{s}'] = points[s], boxes[s], labels3[s], labels10[s]
    n = sum(len(p) for p in points)

    heads = {'sig': dict(use_sigmoid=True, num_classes=3, labels=labels3),
             'ce': dict(use_sigmoid=False, num_classes=10, labels=labels10)}
    targets = {}
    for case, spec in heads.items():
        for tag, width in WIDTHS.items():
            cfg = {} if width is None else {'extra_width': width}
            head = make_head(spec['use_sigmoid'], spec['num_classes'], cfg)
            lab, tgt, mask = reference_targets(head, [p[:, :3] for p in points], boxes, spec['labels'])
            lab64, tgt64, _ = reference_targets(head, [p[:, :3].astype(np.float64) for p in points],
                                                [b.astype(np.float64) for b in boxes], spec['labels'])
            assert np.array_equal(lab, lab64)
            out[f'tgt_{case}_{tag}_labels'] = lab
            if f'tgt_{tag}_mask' in out:      # the geometry, hence mask and vote targets, is the same for both label sets
                assert np.array_equal(out[f'tgt_{tag}_mask'], mask) and np.array_equal(out[f'tgt_{tag}_targets'], tgt)
            out[f'tgt_{tag}_targets'], out[f'tgt_{tag}_targets64'], out[f'tgt_{tag}_mask'] = tgt, tgt64, mask
            targets[case, tag] = (lab, tgt, mask)
        assert not np.array_equal(targets[case, 'none'][0], targets[case, 'p02'][0])
        assert not np.array_equal(targets[case, 'none'][0], targets[case, 'm03'][0])

    # loss cases on the targets without an extra width; inputs exactly representable in float16 (stored as such)
    def f16(x):
        return x.astype(np.float16).astype(np.float32)

    lab, tgt, mask = targets['sig', 'none']
    thr = np.float64(WAYMO_THRESH)
    logits3 = away_from_thresholds(rng, lambda r: f16(r.normal(0, 2.0, (n, 3))),
                                   lambda x: np.abs(1 / (1 + np.exp(-x.astype(np.float64))) - thr[None]).min(1))
    votes3 = f16(rng.normal(0, 1.0, (n, 9)))
    cfg = dict(score_thresh=WAYMO_THRESH, class_names=WAYMO_NAMES)
    head = make_head(True, 3, cfg, gamma=3.0, alpha=0.8)
    runs = {'sig': (head, logits3, votes3, lab, tgt, mask)}

    lab, tgt, mask = targets['ce', 'none']
    grp = np.array(R.class_group(R.NUSC_CLASS_NAMES, R.NUSC_GROUP_NAMES))
    thr10 = np.float64(R.NUSC_SCORE_THRESH)

    def ce_margin(x):
        z = x.astype(np.float64)
        p = np.exp(z - z.max(1, keepdims=True))
        p = (p / p.sum(1, keepdims=True))[:, :-1]
        gs = np.stack([p[:, grp == g].sum(1) for g in range(len(thr10))], 1)
        return np.abs(gs - thr10[None]).min(1)

    logits11 = away_from_thresholds(rng, lambda r: f16(r.normal(0, 2.0, (n, 11))), ce_margin)
    votes11 = f16(rng.normal(0, 1.0, (n, 33)))
    cfg = dict(score_thresh=R.NUSC_SCORE_THRESH, class_names=R.NUSC_CLASS_NAMES, group_names=R.NUSC_GROUP_NAMES)
    head = make_head(False, 10, cfg, class_weight=R.NUSC_CLASS_WEIGHT)
    runs['ce'] = (head, logits11, votes11, lab, tgt, mask)

    for case, (head, logits, votes, lab, tgt, mask) in runs.items():
        out[f'{case}_logits'], out[f'{case}_vote_preds'] = logits.astype(np.float16), votes.astype(np.float16)
        r32 = reference_losses(head, logits, votes, lab, tgt, mask, torch.float32)
        r64 = reference_losses(head, logits, votes, lab, tgt, mask, torch.float64)
        for k in r64:
            out[f'{case}_f32_{k}'], out[f'{case}_f64_{k}'] = r32[k], r64[k]
            if k.startswith('loss'):
                out[f'noise_{case}_{k}'] = np.abs(r32[k].astype(np.float64) - r64[k]) / np.abs(r64[k])
            elif k.startswith('d_'):
                out[f'noise_{case}_{k}'] = np.abs(r32[k].astype(np.float64) - r64[k]).max() / np.abs(r64[k]).max()
        print(case, {k: (v.reshape(-1)[:3] if v.size > 3 else v) for k, v in r64.items() if not k.startswith('d_')})
        print('   noise', {k: float(np.max(v)) for k, v in out.items() if k.startswith(f'noise_{case}')})
    path = os.path.join(ROOT, 'tests', 'golden', 'seg_head_train.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
