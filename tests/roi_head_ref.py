"""The fused data flow of the RoI head (csrc/roi_head.hip, sst_amd/roi_head.py) restated in torch on the CPU, in float32 or
float64, for tests/test_roi_head_host.py, tests/test_gpu_roi_head.py and tests/golden/make_roi_head_train.py.

- overlaps3d: BaseInstance3DBoxes.overlaps with the BEV overlap of tests/box_ops_ref.py (float32: the reference's polygon
  algorithm operation by operation; float64: an independent clip).
- assign_sample: the masked IoU matrix, row maximum / first arg-maximum, mmdet's assign_wrt_overlaps with gt_max_assign_all, the
  IoUNegPiecewiseSampler with "k of a pool = its k smallest (key, index)", and the padded per-sample rows with soft labels and
  the regression targets of _get_target_single.
- losses: FullySparseBboxHead.loss as one expression per loss, differentiable by autograd.
- decode: decode_from_rois, the sigmoid and the xyxyr rows.
"""
import numpy as np
import torch

import box_ops_ref as B

WAYMO_NAMES = ['Car', 'Pedestrian', 'Cyclist']
# configs/fsd/fsd_waymoD1_1x.py: train_cfg.rcnn
WAYMO_CFG = dict(num_classes=3, class_mask=True, pos_iou_thr=[0.45, 0.35, 0.35], neg_iou_thr=[0.45, 0.35, 0.35],
                 min_pos_iou=[0.45, 0.35, 0.35], num=256, pos_fraction=0.55, neg_piece_fractions=[0.8, 0.2],
                 neg_iou_piece_thrs=[0.55, 0.1], cls_pos_thr=(0.8, 0.65, 0.65), cls_neg_thr=(0.2, 0.15, 0.15))
ROW_KEYS = ('rois', 'src', 'gt_index', 'labels', 'iou', 'soft_label', 'reg_mask', 'targets')
TWO_PI = 2 * np.pi


def with_cfg(**over):
    cfg = dict(WAYMO_CFG)
    cfg.update(over)
    return cfg


def bev_rows(boxes):
    """xywhr2xyxyr(LiDARInstance3DBoxes.bev) in the dtype of ``boxes``"""
    hw, hl = boxes[:, 3] / 2, boxes[:, 4] / 2
    return np.stack([boxes[:, 0] - hw, boxes[:, 1] - hl, boxes[:, 0] + hw, boxes[:, 1] + hl, boxes[:, 6]], 1)


def bev_matrix(ra, rb, dtype=np.float32, cap=True):
    """[N, 5] x [M, 5] xyxyr rows -> [N, M] rotated overlap areas.  float32: the reference's polygon algorithm operation by
    operation (cap: with the library's one departure from it, csrc/bev_clip.h - an overlap cannot exceed either box); float64: an
    independent clip of the pairs whose circumscribed circles meet"""
    if dtype == np.float32:
        bev = B.pairwise(B.bev_overlap_f32, ra, rb)
        if cap:
            bev = np.minimum(bev, np.minimum(np.abs((ra[:, 2] - ra[:, 0]) * (ra[:, 3] - ra[:, 1]))[:, None],
                                             np.abs((rb[:, 2] - rb[:, 0]) * (rb[:, 3] - rb[:, 1]))[None]))
        return bev.astype(np.float32)
    bev = np.zeros((len(ra), len(rb)))
    ca, cb = (ra[:, 0:2] + ra[:, 2:4]) / 2, (rb[:, 0:2] + rb[:, 2:4]) / 2
    da, db = np.hypot(ra[:, 2] - ra[:, 0], ra[:, 3] - ra[:, 1]), np.hypot(rb[:, 2] - rb[:, 0], rb[:, 3] - rb[:, 1])
    near = np.hypot(ca[:, 0][:, None] - cb[:, 0][None], ca[:, 1][:, None] - cb[:, 1][None]) <= 0.5 * (da[:, None] + db[None]) + 0.05
    for i, j in zip(*np.nonzero(near)):
        bev[i, j] = B.bev_overlap_f64(ra[i], rb[j])
    return bev


def overlaps3d(boxes1, boxes2, dtype=np.float32):
    """[N, >= 7] x [M, >= 7] -> [N, M] 3-D IoU (BaseInstance3DBoxes.overlaps, mode 'iou')"""
    a, b = np.asarray(boxes1)[:, :7].astype(dtype), np.asarray(boxes2)[:, :7].astype(dtype)
    if len(a) * len(b) == 0:
        return np.zeros((len(a), len(b)), dtype)
    bev = bev_matrix(bev_rows(a), bev_rows(b), dtype)
    top = np.minimum((a[:, 2] + a[:, 5])[:, None], (b[:, 2] + b[:, 5])[None])
    bottom = np.maximum(a[:, 2][:, None], b[:, 2][None])
    o3 = bev.astype(dtype) * np.maximum(top - bottom, dtype(0))
    v1, v2 = (a[:, 3] * a[:, 4] * a[:, 5])[:, None], (b[:, 3] * b[:, 4] * b[:, 5])[None]
    return (o3 / np.maximum(v1 + v2 - o3, dtype(1e-8))).astype(dtype)


def target_rows(roi, gt, dtype=torch.float32):
    """_get_target_single's canonical transform and DeltaXYZWLHRBBoxCoder.encode for paired rows [K, 7] -> [K, 7]"""
    roi, gt = torch.as_tensor(roi)[:, :7].to(dtype), torch.as_tensor(gt)[:, :7].to(dtype)
    ct = gt.clone()
    roi_ry = roi[:, 6] % TWO_PI
    ct[:, 0:3] -= roi[:, 0:3]
    ct[:, 6] -= roi_ry
    ang = -(roi_ry + np.pi / 2)
    sn, cs = torch.sin(ang), torch.cos(ang)
    x, y = ct[:, 0] * cs + ct[:, 1] * sn, -ct[:, 0] * sn + ct[:, 1] * cs
    ry = ct[:, 6] % TWO_PI
    opposite = (ry > np.pi * 0.5) & (ry < np.pi * 1.5)
    ry = torch.where(opposite, (ry + np.pi) % TWO_PI, ry)
    ry = torch.where(ry > np.pi, ry - np.pi * 2, ry)
    ry = torch.clamp(ry, min=-np.pi / 2, max=np.pi / 2)
    wa, la, ha = roi[:, 3], roi[:, 4], roi[:, 5]
    diag = torch.sqrt(la ** 2 + wa ** 2)
    zt = ((ct[:, 2] + gt[:, 5] / 2) - ha / 2) / ha
    return torch.stack([x / diag, y / diag, zt, torch.log(gt[:, 3] / wa), torch.log(gt[:, 4] / la), torch.log(gt[:, 5] / ha), ry], 1)


def canonical_yaw(roi, gt):
    """the yaw label before the flip, in float64 (for the scene's distance from pi / 2, pi, 3 pi / 2)"""
    roi, gt = np.asarray(roi, np.float64), np.asarray(gt, np.float64)
    return (gt[:, 6] - roi[:, 6] % TWO_PI) % TWO_PI


def fake_box(cols):
    return np.array([[0, 0, 5, 1, 1, 1, 0] + [0] * (cols - 7)], np.float32)


def with_fake_boxes(props, plabels):
    """fsd_roi_head.py:232-241: a sample without a proposal gets one box with label 0"""
    cols = props[0].shape[1]
    props, plabels = list(props), list(plabels)
    for s in range(len(props)):
        if len(props[s]) == 0:
            props[s], plabels[s] = fake_box(cols), np.zeros(1, np.int64)
    return props, plabels


def choose(pool, k, keys):
    """the k smallest (key, index) of a pool of indices"""
    pool = np.asarray(pool, np.int64)
    if len(pool) <= k:
        return pool
    order = np.lexsort((pool, keys[pool]))
    return np.sort(pool[order[:k]])


def assign_sample(props, plabels, gts, glabels, cfg, keys, dtype=np.float32, overlap_fn=overlaps3d):
    """-> dict of numpy arrays named as ``sst_amd.roi_assign_sample`` names them (padded rows, counts [B, 2], overlaps [P, ld],
    max_overlaps, argmax, assigned).  keys: float32 [sum P_i] with the fake boxes included."""
    props, plabels = with_fake_boxes([np.asarray(p, np.float32) for p in props], [np.asarray(l, np.int64) for l in plabels])
    gts, glabels = [np.asarray(g, np.float32) for g in gts], [np.asarray(l, np.int64) for l in glabels]
    batch, cols, num, nc = len(props), props[0].shape[1], cfg['num'], cfg['num_classes']
    ld = max(len(g) for g in gts)
    n_props = sum(len(p) for p in props)
    keys = np.asarray(keys, np.float32)
    assert keys.shape == (n_props,)
    cfg = dict(cfg)
    for name in ('pos_iou_thr', 'neg_iou_thr', 'min_pos_iou', 'cls_pos_thr', 'cls_neg_thr'):      # a float is broadcast
        if not isinstance(cfg[name], (list, tuple)):
            cfg[name] = [cfg[name]] * nc
    thr = lambda name, c: dtype(cfg[name][c if cfg['class_mask'] else 0])                             # noqa: E731
    out = dict(rois=np.zeros((batch * num, 1 + cols), np.float32), src=np.full(batch * num, -1, np.int32),
               gt_index=np.full(batch * num, -1, np.int32), labels=np.full(batch * num, -1, np.int64),
               iou=np.zeros(batch * num, dtype), soft_label=np.zeros(batch * num, dtype),
               reg_mask=np.zeros(batch * num, np.uint8), targets=np.zeros((batch * num, 7), dtype),
               counts=np.zeros((batch, 2), np.int32), overlaps=np.full((n_props, ld), -1, dtype),
               max_overlaps=np.zeros(n_props, dtype), argmax=np.full(n_props, -1, np.int32),
               assigned=np.full(n_props, -1, np.int32), pool_sizes=[])
    p0 = g0 = 0
    for s in range(batch):
        p, pl, g, gl = props[s], plabels[s], gts[s], glabels[s]
        n, m = len(p), len(g)
        pv, gv = (pl >= 0) & (pl < nc), (gl >= 0) & (gl < nc)
        mask = pv[:, None] & gv[None]
        if cfg['class_mask']:
            mask &= pl[:, None] == gl[None]
        mat = np.where(mask, overlap_fn(p, g, dtype) if m else np.zeros((n, 0), dtype), dtype(-1))
        out['overlaps'][p0:p0 + n, :m] = mat
        any_gt = mask.any(1)
        am = np.where(any_gt, mat.argmax(1) if m else 0, -1)
        mx = np.where(any_gt, mat.max(1) if m else 0, 0).astype(dtype)
        assigned = np.full(n, -2, np.int64)
        for i in range(n):
            if not any_gt[i]:
                assigned[i] = -1
                continue
            if 0 <= mx[i] < thr('neg_iou_thr', pl[i]):
                assigned[i] = -1
            if mx[i] >= thr('pos_iou_thr', pl[i]):
                assigned[i] = am[i]
        for j in range(m):
            col = mat[:, j]
            if gv[j] and col.max(initial=-1) >= 0 and col.max() >= thr('min_pos_iou', gl[j]):
                assigned[col == col.max()] = j
        out['max_overlaps'][p0:p0 + n], out['argmax'][p0:p0 + n] = mx, np.where(am >= 0, am + g0, -1)
        out['assigned'][p0:p0 + n] = np.where(assigned >= 0, assigned + g0, assigned)
        # IoUNegPiecewiseSampler.sample
        k = keys[p0:p0 + n]
        pos_pool, neg_pool = np.nonzero(assigned >= 0)[0], np.nonzero(assigned == -1)[0]
        pos = choose(pos_pool, int(num * cfg['pos_fraction']), k)
        expected = num - len(pos)
        sizes = [len(pos_pool)]
        if len(neg_pool) <= expected:
            neg = neg_pool
            sizes.append(len(neg_pool))
        else:
            chosen, extend, pieces = [], 0, cfg['neg_iou_piece_thrs']
            for q in range(len(pieces)):
                last = q == len(pieces) - 1
                want = expected - sum(len(c) for c in chosen) if last else int(expected * cfg['neg_piece_fractions'][q]) + extend
                lo = dtype(0) if last else dtype(pieces[q + 1])
                piece = neg_pool[(mx[neg_pool] >= lo) & (mx[neg_pool] < dtype(pieces[q]))]
                sizes.append(len(piece))
                if len(piece) < want:
                    chosen.append(piece)
                    extend += want - len(piece)
                else:
                    chosen.append(choose(piece, max(want, 0), k))
                    extend = 0
            neg = np.unique(np.concatenate(chosen))
        out['pool_sizes'].append(sizes)
        out['counts'][s] = (len(pos), len(neg))
        rows = np.concatenate([pos, neg]).astype(np.int64)
        o = s * num + np.arange(len(rows))
        out['rois'][o, 0], out['rois'][o, 1:] = s, p[rows]
        out['src'][o] = rows + p0
        out['iou'][o] = mx[rows]
        op = o[:len(pos)]
        if len(pos):
            a = assigned[pos]
            out['gt_index'][op], out['labels'][op], out['reg_mask'][op] = a + g0, gl[a], 1
            out['targets'][op] = target_rows(p[pos], g[a], torch.float32 if dtype == np.float32 else torch.float64).numpy()
            cp = np.asarray([cfg['cls_pos_thr'][c] for c in gl[a]], np.float64)
            cn = np.asarray([cfg['cls_neg_thr'][c] for c in gl[a]], np.float64)
            iou = mx[pos]
            soft = (iou - cn.astype(dtype)) / (cp - cn).astype(dtype)
            out['soft_label'][op] = np.where(iou > cp.astype(dtype), 1, np.where(iou < cn.astype(dtype), 0, soft))
        p0, g0 = p0 + n, g0 + m
    return out


def compact(res):
    """drop the padding rows, as ``sst_amd.roi_compact`` does"""
    num = len(res['src']) // len(res['counts'])
    rows = np.concatenate([np.arange(s * num, s * num + c[0] + c[1]) for s, c in enumerate(res['counts'])])
    out = dict(res)
    for k in ROW_KEYS:
        out[k] = res[k][rows]
    return out


def rotate_z(xyz, angle):
    """rotation_3d_in_axis(axis=2) of one point per row"""
    c, s = torch.cos(angle), torch.sin(angle)
    return torch.stack([xyz[:, 0] * c + xyz[:, 1] * s, -xyz[:, 0] * s + xyz[:, 1] * c, xyz[:, 2]], 1)


def decode_rows(roi, pred):
    """DeltaXYZWLHRBBoxCoder.decode against the zero-centred RoI, the rotation by roi_ry + pi / 2, the RoI centre: [K, 7]"""
    wa, la, ha, ra = roi[:, 3], roi[:, 4], roi[:, 5], roi[:, 6]
    diag = torch.sqrt(la ** 2 + wa ** 2)
    hg = torch.exp(pred[:, 5]) * ha
    local = torch.stack([pred[:, 0] * diag, pred[:, 1] * diag, pred[:, 2] * ha + ha / 2 - hg / 2], 1)
    xyz = rotate_z(local, ra + np.pi / 2) + roi[:, 0:3]
    return torch.cat([xyz, (torch.exp(pred[:, 3]) * wa)[:, None], (torch.exp(pred[:, 4]) * la)[:, None], hg[:, None],
                      (pred[:, 6] + ra)[:, None]], 1)


CORNERS = torch.tensor([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1], [1, 1, 0]]) \
    - torch.tensor([0.5, 0.5, 0])


def corners(boxes):
    """LiDARInstance3DBoxes.corners: [K, 7] -> [K, 8, 3]"""
    local = boxes[:, None, 3:6] * CORNERS.to(boxes.dtype)[None]
    c, s = torch.cos(boxes[:, 6])[:, None], torch.sin(boxes[:, 6])[:, None]
    x, y = local[..., 0] * c + local[..., 1] * s, -local[..., 0] * s + local[..., 1] * c
    return torch.stack([x, y, local[..., 2]], -1) + boxes[:, None, 0:3]


def corner_distances(pred_boxes, gt_boxes):
    """-> (distance to the box's corners, to the flipped box's corners), each [K, 8]"""
    flip = gt_boxes.clone()
    flip[:, 6] += np.pi
    pc = corners(pred_boxes)
    return torch.norm(pc - corners(gt_boxes), dim=2), torch.norm(pc - corners(flip), dim=2)


def losses(cls_score, bbox_pred, nonempty, rows, gts, *, loss_weights=(1.0, 2.0, 1.0), beta=0.0, code_weight=None,
           with_corner=True, car_index=0, upstream=(1.0, 1.0, 1.0), dtype=torch.float64):
    """FullySparseBboxHead.loss on compacted rows -> dict(loss_cls, loss_bbox, loss_corner, num_pos, num_neg, corner_rows,
    d_cls [R, 1], d_bbox [R, 7]); the gradients are those of sum(upstream_k * loss_k)"""
    z = torch.as_tensor(cls_score).to(dtype).reshape(-1).clone().requires_grad_(True)
    bp = torch.as_tensor(bbox_pred).to(dtype).clone().requires_grad_(True)
    nonempty = torch.as_tensor(np.asarray(nonempty).astype(bool))
    soft, tg = torch.as_tensor(rows['soft_label']).to(dtype), torch.as_tensor(rows['targets']).to(dtype)
    roi = torch.as_tensor(rows['rois'])[:, 1:8].to(dtype)
    reg = torch.as_tensor(rows['reg_mask'].astype(bool)) & nonempty
    n = len(z)
    bce = torch.clamp(z, min=0) - z * soft + torch.log1p(torch.exp(-z.abs()))
    loss_cls = loss_weights[0] * (bce * nonempty).sum() / n
    num_pos = int(reg.sum())
    zero = bp.sum() * 0
    loss_bbox = loss_corner = zero
    corner_rows = 0
    if num_pos:
        d = (bp[reg] - tg[reg]).abs()
        elem = torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta) if beta > 0 else d
        if code_weight is not None:
            elem = elem * torch.as_tensor(code_weight).to(dtype)[None]
        loss_bbox = loss_weights[1] * elem.sum() / num_pos
        if with_corner:
            keep = reg.clone()
            if car_index >= 0:
                keep &= torch.as_tensor(rows['labels'] == car_index)
            corner_rows = int(keep.sum())
            if corner_rows:
                gt = torch.as_tensor(gts)[torch.as_tensor(rows['gt_index'][keep.numpy()].astype(np.int64)), :7].to(dtype)
                d0, d1 = corner_distances(decode_rows(roi[keep], bp[keep]), gt)
                dist = torch.min(d0, d1)
                quad = torch.clamp(dist, max=1)
                loss_corner = loss_weights[2] * (0.5 * quad ** 2 + (dist - quad)).mean()
    total = upstream[0] * loss_cls + upstream[1] * loss_bbox + upstream[2] * loss_corner
    total.backward()
    return dict(loss_cls=float(loss_cls.detach()), loss_bbox=float(loss_bbox.detach()), loss_corner=float(loss_corner.detach()), num_pos=num_pos,
                num_neg=n - num_pos, corner_rows=corner_rows, d_cls=z.grad.reshape(-1, 1).numpy(), d_bbox=bp.grad.numpy())


def decode(rois, bbox_pred, cls_score, dtype=torch.float64):
    """-> (boxes [R, cols], scores [R], bev [R, 5])"""
    rois, bp = torch.as_tensor(rois).to(dtype), torch.as_tensor(bbox_pred).to(dtype)
    boxes = torch.cat([decode_rows(rois[:, 1:8], bp), rois[:, 8:]], 1)
    bev = torch.as_tensor(bev_rows(boxes.numpy()))
    return boxes.numpy(), torch.sigmoid(torch.as_tensor(cls_score).to(dtype).reshape(-1)).numpy(), bev.numpy()


# ---- scenes ----------------------------------------------------------------------------------------------------------

def random_boxes(rng, n, cols, extent):
    b = np.zeros((n, cols), np.float32)
    b[:, 0:2] = rng.uniform(-extent, extent, (n, 2))
    b[:, 2] = rng.uniform(-1.5, -0.5, n)
    b[:, 3] = rng.uniform(0.6, 2.2, n)
    b[:, 4] = rng.uniform(0.8, 5.0, n)
    b[:, 5] = rng.uniform(1.2, 2.0, n)
    b[:, 6] = rng.uniform(-2 * np.pi, 2 * np.pi, n)
    if cols > 7:
        b[:, 7:] = rng.normal(0, 2, (n, cols - 7))
    return b


def make_scene(seed, prop_lens, gt_lens, cols=7, gt_cols=7, num_classes=3, extent=25.0):
    """proposals scattered around the boxes of their sample (six in ten are jittered copies of a box, most with its label),
    a few boxes labelled -1 and a few proposals with a label outside the classes"""
    rng = np.random.default_rng(seed)
    props, plabels, gts, glabels = [], [], [], []
    for n, m in zip(prop_lens, gt_lens):
        g = random_boxes(rng, m, gt_cols, extent)
        gl = rng.integers(0, num_classes, m)
        if m > 3:
            gl[rng.integers(0, m)] = -1
        p = random_boxes(rng, n, cols, extent)
        pl = rng.integers(0, num_classes, n)
        if m and n:
            near = rng.random(n) < 0.6
            of = rng.integers(0, m, n)
            scale = rng.choice([0.02, 0.1, 0.3, 0.6], n)[:, None]
            jit = rng.normal(0, 1, (n, 7)) * np.array([0.8, 0.8, 0.3, 0.3, 0.5, 0.2, 0.3]) * scale
            p[near, :7] = (g[of, :7] + jit)[near].astype(np.float32)
            p[:, 3:6] = np.maximum(p[:, 3:6], 0.3)
            same = near & (rng.random(n) < 0.85) & (gl[of] >= 0)
            pl[same] = gl[of][same]
        if n > 5:
            pl[rng.integers(0, n)] = num_classes + 1
            pl[rng.integers(0, n)] = -1
        props.append(p), plabels.append(pl.astype(np.int64)), gts.append(g), glabels.append(gl.astype(np.int64))
    return props, plabels, gts, glabels


def make_keys(seed, props):
    n = sum(max(len(p), 1) for p in props)
    return np.random.default_rng(seed).random(n, dtype=np.float32)


def make_predictions(seed, n, nonempty_fraction=0.85):
    """cls_score [n, 1], bbox_pred [n, 7] (small deltas, as a trained head emits them), nonempty bool [n]"""
    rng = np.random.default_rng(seed)
    return (rng.normal(-1, 2, (n, 1)).astype(np.float32),
            (rng.normal(0, 1, (n, 7)) * np.array([0.3, 0.3, 0.3, 0.2, 0.2, 0.2, 0.4])).astype(np.float32),
            rng.random(n) < nonempty_fraction)
