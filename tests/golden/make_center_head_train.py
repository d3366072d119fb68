"""Generates tests/golden/center_head_train.npz: CenterHead's targets, losses and box decoding as the REFERENCE computes them
(data only).

Needs the reference tree (oracle.ref_loader); run from the repository root:  python tests/golden/make_center_head_train.py

Executed from their source text: CenterHead.get_targets_single / get_targets / loss / _gather_feat
(mmdet3d/models/dense_heads/centerpoint_head.py), gaussian_radius / draw_heatmap_gaussian / gaussian_2d
(mmdet3d/core/utils/gaussian.py), clip_sigmoid (mmdet3d/models/utils/clip_sigmoid.py), CenterPointBBoxCoder with decode and its
helpers (mmdet3d/core/bbox/coders/centerpoint_bbox_coders.py) and LiDARInstance3DBoxes.gravity_center
(mmdet3d/core/bbox/structures/lidar_box3d.py).  What the reference imports from packages that are not in its tree is stood in
for here:
  mmdet GaussianFocalLoss   (-(p + 1e-12).log() (1 - p)^2 [t == 1] - (1 - p + 1e-12).log() p^2 (1 - t)^4).sum() / avg_factor
                            x loss_weight: mmdet 2.x gaussian_focal_loss with alpha 2, gamma 4, reduction 'mean'
  mmdet L1Loss              (|pred - target| * weight).sum() / avg_factor x loss_weight (reduction 'mean' with avg_factor)
  mmdet multi_apply         tuple(map(list, zip(*map(func, *args))))
  mmcv force_fp32           dropped with the decorators (the inputs are of one dtype already)
  mmdet BaseBBoxCoder       object
Each loss case is run in float32 and in float64; noise_* is the gap between the two runs relative to the tensor's maximum.
The loss runs hand the reference a copy of the logits: its clip_sigmoid works in place.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import center_head_ref as R  # noqa: E402
from center_head_ref import (CASES, CELL, DECODE_CASES, H, LOSS_CASES, MAX_NUM, PC, POST_CENTER_RANGE, W, W_BBOX, W_CLS,  # noqa: E402
                             coder_cfg)

HEAD_PY = 'mmdet3d/models/dense_heads/centerpoint_head.py'
GAUSS_PY = 'mmdet3d/core/utils/gaussian.py'
CLIP_PY = 'mmdet3d/models/utils/clip_sigmoid.py'
CODER_PY = 'mmdet3d/core/bbox/coders/centerpoint_bbox_coders.py'
BOX_PY = 'mmdet3d/core/bbox/structures/lidar_box3d.py'

_CACHE = {}


def reference_parts():
    if _CACHE:
        return _CACHE
    from oracle import ref_loader
    g2d = ref_loader.load_reference_function(GAUSS_PY, 'gaussian_2d', {'np': np})
    _CACHE['gaussian_2d'] = g2d
    _CACHE['draw_heatmap_gaussian'] = ref_loader.load_reference_function(GAUSS_PY, 'draw_heatmap_gaussian',
                                                                         {'np': np, 'gaussian_2d': g2d})
    _CACHE['gaussian_radius'] = ref_loader.load_reference_function(GAUSS_PY, 'gaussian_radius')
    _CACHE['clip_sigmoid'] = ref_loader.load_reference_function(CLIP_PY, 'clip_sigmoid')
    glb = {'draw_heatmap_gaussian': _CACHE['draw_heatmap_gaussian'], 'gaussian_radius': _CACHE['gaussian_radius'],
           'clip_sigmoid': _CACHE['clip_sigmoid'], 'multi_apply': lambda f, *a: tuple(map(list, zip(*map(f, *a))))}
    for name in ('get_targets_single', 'get_targets', 'loss', '_gather_feat'):
        _CACHE[name] = ref_loader.load_reference_method(HEAD_PY, 'CenterHead', name, glb)
    _CACHE['gravity_center'] = ref_loader.load_reference_method(BOX_PY, 'LiDARInstance3DBoxes', 'gravity_center')
    _CACHE['coder'] = ref_loader.load_reference_class(CODER_PY, 'CenterPointBBoxCoder', {'BaseBBoxCoder': object})
    return _CACHE


class Boxes(object):
    """what get_targets_single asks of a LiDARInstance3DBoxes"""

    def __init__(self, tensor):
        self.tensor = tensor

    bottom_center = property(lambda self: self.tensor[:, :3])
    gravity_center = property(lambda self: reference_parts()['gravity_center'](self))


def make_head(cfg, tasks, norm_bbox):
    """a stand-in ``self`` for the reference's methods"""
    parts = reference_parts()
    head = types.SimpleNamespace()
    head.train_cfg, head.norm_bbox = cfg, norm_bbox
    head.class_names = [t['class_names'] for t in tasks]
    head.task_heads = [None] * len(tasks)
    for name in ('get_targets_single', 'get_targets', 'loss', '_gather_feat'):
        setattr(head, name, types.MethodType(parts[name], head))
    head.loss_cls = lambda pred, target, avg_factor: W_CLS * R.gaussian_focal_terms(pred, target.to(pred.dtype)).sum() / avg_factor
    head.loss_bbox = lambda pred, target, weight, avg_factor: W_BBOX * ((pred - target).abs() * weight).sum() / avg_factor
    return head


def make_scene(rng):
    """three samples of 9-column boxes and labels; the middle one has no boxes"""
    def centre(cx, cy, dx=0.0, dy=0.0):
        return [PC[0] + (cx + 0.5) * CELL + dx, PC[1] + (cy + 0.5) * CELL + dy]

    def random_boxes(n):
        b = np.zeros((n, 9), np.float32)
        kind = rng.integers(0, 3, n)
        b[:, 0] = rng.uniform(PC[0] + 0.4, PC[3] - 0.4, n)
        b[:, 1] = rng.uniform(PC[1] + 0.4, PC[4] - 0.4, n)
        b[:, 2] = rng.uniform(-1.5, -0.5, n)
        size = np.float32([[2.0, 4.6, 1.6], [0.8, 0.9, 1.7], [0.8, 1.8, 1.7]])[kind]    # boxes of under ~3 cells: min_radius decides
        b[:, 3:6] = size * rng.uniform(0.8, 1.25, (n, 3))
        b[:, 6] = rng.uniform(-np.pi, np.pi, n)
        b[:, 7:9] = rng.normal(0, 2.0, (n, 2))
        return b, kind.astype(np.int64)

    scenes = []
    for s in range(2):
        b, lab = random_boxes(30)
        if s == 0:
            car, big = [2.0, 4.6, 1.6], [3.0, 7.5, 2.5]
            b[0, :2], b[0, 3:6] = centre(0, 17), big                    # clipped at the left border
            b[1, :2], b[1, 3:6] = centre(39, 9), big                    # right
            b[2, :2], b[2, 3:6] = centre(20, 0), big                    # top
            b[3, :2], b[3, 3:6] = centre(12, 35), big                   # bottom
            b[4, :2], b[4, 3:6] = centre(38, 34), big                   # a corner
            lab[:5] = 0
            b[5, :2], b[6, :2] = centre(10, 10, -0.05, 0.04), centre(10, 10, 0.06, -0.03)    # one class, one cell
            b[5, 3:6], b[6, 3:6] = car, [1.9, 4.2, 1.5]
            lab[5] = lab[6] = 0
            b[7, :2], b[8, :2] = centre(25, 20, 0.02, 0.05), centre(25, 20, -0.07, -0.06)    # two classes, one cell
            lab[7], lab[8] = 1, 2
            lab[9] = lab[10] = -1
            b[11, :2] = [PC[0] - 0.1, PC[1] + 3.0]                       # coor_x in (-1, 0): cell 0, kept
            b[12, :2] = [PC[3] + 0.5, PC[1] + 5.0]                       # outside on the high side: dropped
            b[13, 3] = 0.0                                               # zero width: skipped, keeps its rank
            lab[11], lab[12], lab[13] = 1, 0, 0
        scenes.append((b, lab))
    empty = (np.zeros((0, 9), np.float32), np.zeros((0,), np.int64))
    return [scenes[0], empty, scenes[1]]


def reference_targets(head, boxes, labels):
    hm, anno, ind, mask = head.get_targets([Boxes(torch.as_tensor(b)) for b in boxes], [torch.as_tensor(l) for l in labels])
    return [[t.numpy() for t in lst] for lst in (hm, anno, ind, mask)]


def reference_loss(head, boxes, labels, logits, heads, task_channels, dtype):
    """-> per task dict(loss_heatmap, loss_bbox, d_logits, d_heads) from the reference's loss in ``dtype``"""
    lg = torch.as_tensor(logits).to(dtype).requires_grad_(True)
    hs = [torch.as_tensor(h).to(dtype).requires_grad_(True) for h in heads]
    preds, at = [], 0
    for c in task_channels:
        d = dict(zip(('reg', 'height', 'dim', 'rot', 'vel'), hs))
        d['heatmap'] = lg[:, at:at + c] * 1      # a copy: clip_sigmoid works in place
        preds.append([d])
        at += c
    out = head.loss([Boxes(torch.as_tensor(b)) for b in boxes], [torch.as_tensor(l) for l in labels], preds)
    res = []
    for t in range(len(task_channels)):
        for h in [lg] + hs:
            h.grad = None
        (out[f'task{t}.loss_heatmap'] + out[f'task{t}.loss_bbox']).backward(retain_graph=True)
        res.append(dict(loss_heatmap=out[f'task{t}.loss_heatmap'].detach().numpy(),
                        loss_bbox=out[f'task{t}.loss_bbox'].detach().numpy(), d_logits=lg.grad.numpy().copy(),
                        d_heads=np.concatenate([h.grad.numpy() for h in hs], 1)))
    return res


def main():
    rng = np.random.default_rng(20261)
    parts = reference_parts()
    out = {}
    scene = make_scene(rng)
    for s, (b, lab) in enumerate(scene):
        out[f'boxes{s}'], out[f'labels{s}'] = b, lab
    labels = [lab for _, lab in scene]

    heads_of = {}
    for case, (cfg, tasks, norm_bbox, cols) in CASES.items():
        boxes = [b[:, :cols] for b, _ in scene]
        head = heads_of[case] = make_head(cfg, tasks, norm_bbox)
        hm, anno, ind, mask = reference_targets(head, boxes, labels)
        for t in range(len(tasks)):
            out[f'tgt_{case}_t{t}_heatmap'], out[f'tgt_{case}_t{t}_anno'] = hm[t], anno[t]
            out[f'tgt_{case}_t{t}_ind'], out[f'tgt_{case}_t{t}_mask'] = ind[t], mask[t]
            print(case, t, 'slots', int(mask[t].sum()), 'peaks', int((hm[t] == 1).sum()), 'cells > 0', int((hm[t] > 0).sum()))
    m = out['tgt_shipped_t0_mask'][0].astype(bool)
    cells, n = np.unique(out['tgt_shipped_t0_ind'][0][m], return_counts=True)
    assert (n > 1).sum() >= 2, 'two pairs of slots must share a cell'
    assert out['tgt_max8_t0_mask'].sum() < out['tgt_shipped_t0_mask'].sum()

    # loss and decode inputs: continuous logits with cells beyond both clamp bounds, head maps on a grid of eighths
    logits = rng.normal(0, 3.0, (3, 3, H, W)).astype(np.float32)
    far = rng.choice(logits.size, 60, replace=False)
    logits.reshape(-1)[far] = (rng.uniform(9.5, 12.0, 60) * np.where(np.arange(60) % 2, 1, -1)).astype(np.float32)
    assert (np.abs(np.abs(logits) - 9.21024) > 1e-3).all(), 'a logit at a clamp bound'
    maps = (np.round(rng.normal(0, 1.0, (3, 10, H, W)) * 8) / 8).astype(np.float32)
    out['logits'], out['head_maps'] = logits, maps.astype(np.float16)
    assert np.array_equal(maps, out['head_maps'].astype(np.float32))

    for case in LOSS_CASES:
        cfg, tasks, norm_bbox, cols = CASES[case]
        boxes = [b[:, :cols] for b, _ in scene]
        chans = [len(t['class_names']) for t in tasks]
        r32 = reference_loss(heads_of[case], boxes, labels, logits, R.split_heads(maps), chans, torch.float32)
        r64 = reference_loss(heads_of[case], boxes, labels, logits, R.split_heads(maps), chans, torch.float64)
        for t in range(len(tasks)):
            for k in ('loss_heatmap', 'loss_bbox'):
                out[f'loss_{case}_t{t}_f32_{k}'], out[f'loss_{case}_t{t}_f64_{k}'] = r32[t][k], r64[t][k]
                out[f'noise_{case}_t{t}_{k}'] = np.abs(r32[t][k].astype(np.float64) - r64[t][k]) / np.abs(r64[t][k])
            for k in ('d_logits', 'd_heads'):
                out[f'noise_{case}_t{t}_{k}'] = np.abs(r32[t][k].astype(np.float64) - r64[t][k]).max() / np.abs(r64[t][k]).max()
            # the reference's float64 gradients: every eighth logit gradient and the sum of the magnitudes of all of them; the
            # head gradients in full (they are sparse)
            out[f'loss_{case}_t{t}_f64_d_logits_8th'] = r64[t]['d_logits'].reshape(-1)[::8]
            out[f'loss_{case}_t{t}_f64_d_logits_abs'] = np.abs(r64[t]['d_logits']).sum()
            out[f'loss_{case}_t{t}_f64_d_heads'] = r64[t]['d_heads']
            print(case, t, {k: float(v) for k, v in r64[t].items() if k.startswith('loss')},
                  'noise', {k: float(out[f'noise_{case}_t{t}_{k}']) for k in ('loss_heatmap', 'loss_bbox', 'd_logits', 'd_heads')})

    heat = R.heat_of(logits)
    top = np.sort(heat.reshape(3, -1), 1)[:, ::-1][:, :MAX_NUM + 5]
    assert (np.diff(top, axis=1) < 0).all(), 'score ties among the selected cells'
    thr = float(np.round(np.median(top[:, :MAX_NUM]), 3))
    assert (np.abs(top - thr) > 1e-6).all(), 'a score at the threshold'
    out['decode_score_threshold'] = np.float64(thr)
    for case, with_vel in DECODE_CASES.items():
        norm_bbox = CASES[case][2]
        reg, hei, dim, rot, vel = [torch.from_numpy(h) for h in R.split_heads(maps)]
        coder = parts['coder'](**coder_cfg(case, thr))
        dim_in = torch.exp(dim) if norm_bbox else dim            # as get_bboxes hands it to the coder
        res = coder.decode(torch.from_numpy(heat), rot[:, 0:1], rot[:, 1:2], hei, dim_in, vel if with_vel else None, reg=reg)
        boxes, _, _, keep = R.decode(heat, reg.numpy(), hei.numpy(), dim.numpy(), rot.numpy(), vel.numpy() if with_vel else None,
                                     coder_cfg(case, thr), norm_bbox)
        rng_lo, rng_hi = np.float32(POST_CENTER_RANGE[:3]), np.float32(POST_CENTER_RANGE[3:])
        assert (np.abs(boxes[..., :3] - rng_lo) > 1e-4).all() and (np.abs(boxes[..., :3] - rng_hi) > 1e-4).all()
        for i, r in enumerate(res):
            assert 0 < len(r['scores']) < MAX_NUM and len(r['scores']) == keep[i].sum()
            out[f'decode_{case}_s{i}_bboxes'] = r['bboxes'].numpy()
            out[f'decode_{case}_s{i}_scores'] = r['scores'].numpy()
            out[f'decode_{case}_s{i}_labels'] = r['labels'].numpy()
        print(case, 'decoded', [len(r['scores']) for r in res], 'threshold', thr)
    path = os.path.join(ROOT, 'tests', 'golden', 'center_head_train.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
