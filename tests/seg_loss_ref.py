"""Restatement of what csrc/seg_loss.hip computes (include/sst_amd.h, "Training side of VoteSegHead"), for the tests:
the point targets in numpy float32 with one rounded operation per step (np.sqrt is correctly rounded), the losses in torch
float64 with the gradients left to autograd.  Nothing here is used by the library."""
import numpy as np
import torch

from head_ref_common import ulp_distance  # noqa: F401  (the tests reach it through this module)

SIGMOID_FOCAL, SOFTMAX_CE = 0, 1
F = np.float32

NUSC_CLASS_NAMES = ['car', 'truck', 'trailer', 'bus', 'construction_vehicle', 'bicycle', 'motorcycle', 'pedestrian',
                    'traffic_cone', 'barrier']
NUSC_GROUP_NAMES = [['car'], ['truck', 'construction_vehicle'], ['bus', 'trailer'], ['barrier'],
                    ['motorcycle', 'bicycle'], ['pedestrian', 'traffic_cone']]
NUSC_SCORE_THRESH = [0.2, 0.2, 0.2, 0.1, 0.1, 0.1]
NUSC_CLASS_WEIGHT = [1.0] * 10 + [0.1]


def class_group(class_names, group_names):
    out = [-1] * len(class_names)
    for gi, g in enumerate(group_names):
        for name in g:
            out[class_names.index(name)] = gi
    return out


def enlarge(boxes, extra_width):
    """enlarged_box_hw (lidar_box3d.py:331-346) on [G, 7] float32: w, l += (float)(2 * extra_width); for a negative width a
    box whose enlarged w or l would be <= 0 keeps its own extents"""
    boxes = np.asarray(boxes, F)
    if extra_width is None:
        return boxes.copy()
    out = boxes.copy()
    out[:, 3:5] = out[:, 3:5] + F(2.0 * extra_width)
    if extra_width < 0:
        bad = (out[:, 3:5] <= 0).any(1)
        out[bad] = boxes[bad]
    return out


def inside(boxes, pts):
    """[G, P] membership: the operations of csrc/pib_test.h in float32, one rounding each"""
    b, p = np.asarray(boxes, F), np.asarray(pts, F)
    cz = b[:, 2] + b[:, 5] * F(0.5)
    rot = (b[:, 6].astype(np.float64) + 1.57079632679489661923).astype(F)
    cosa, sina = np.cos(rot).astype(F), np.sin(rot).astype(F)
    sx = p[None, :, 0] - b[:, None, 0]
    sy = p[None, :, 1] - b[:, None, 1]
    lz = p[None, :, 2] - cz[:, None]
    lx = sx * cosa[:, None] + sy * (-sina[:, None])
    ly = sx * sina[:, None] + sy * cosa[:, None]
    hl, hw, hh = b[:, 4] * F(0.5), b[:, 3] * F(0.5), b[:, 5] * F(0.5)
    return ~(np.abs(lz) > hh[:, None]) & (lx > -hl[:, None]) & (lx < hl[:, None]) & (ly > -hw[:, None]) & (ly < hw[:, None])


def local_to_world(box, lx, ly, fz):
    """points at (lx along the length, ly along the width) from the centre of a box and at fraction fz of its height
    (float64 in, float32 [K, 3] out): the inverse of the rotation of csrc/pib_test.h"""
    b = np.asarray(box, np.float64)
    rot = b[6] + np.pi / 2
    return np.stack([b[0] + lx * np.cos(rot) + ly * np.sin(rot), b[1] - lx * np.sin(rot) + ly * np.cos(rot),
                     b[2] + b[5] * fz], 1).astype(F)


def near_a_face(boxes, pts, widths=(0.2, -0.3), tol=1e-3):
    """points within tol of a face plane of any box, at its own extents or enlarged by any of ``widths`` (float64): where
    float32 and float64, or two cos / sin routines, may disagree about membership - the scenes of the tests avoid them"""
    pts = np.asarray(pts, np.float64)
    bad = np.zeros(len(pts), bool)
    for b in np.asarray(boxes, np.float64).reshape(-1, 7):
        rot = b[6] + np.pi / 2
        sx, sy = pts[:, 0] - b[0], pts[:, 1] - b[1]
        lx, ly = sx * np.cos(rot) - sy * np.sin(rot), sx * np.sin(rot) + sy * np.cos(rot)
        lz = pts[:, 2] - (b[2] + b[5] / 2)
        bad |= np.abs(np.abs(lz) - b[5] / 2) < tol
        for ew in [0.0] + [2.0 * w for w in widths]:
            bad |= (np.abs(np.abs(lx) - (b[4] + ew) / 2) < tol) | (np.abs(np.abs(ly) - (b[3] + ew) / 2) < tol)
    return bad


def encode(delta):
    delta = np.asarray(delta, F)
    return (np.sign(delta) * np.sqrt(np.abs(delta))).astype(F)


def point_targets(points_list, boxes_list, labels_list, bg_label, extra_width=None, centers=None, member=inside):
    """-> (labels int64 [N], vote_targets float32 [N, 3], vote_mask bool [N], inbox int32 [N] into the concatenated boxes).
    centers: optional [G_total, 3] float32 vote centres per box; member(boxes, pts) -> [G, P] bool."""
    labels, targets, masks, inboxes = [], [], [], []
    base = 0
    for pts, boxes, box_labels in zip(points_list, boxes_list, labels_list):
        pts = np.asarray(pts, F)[:, :3]
        boxes = np.asarray(boxes, F).reshape(-1, 7)
        box_labels = np.asarray(box_labels, np.int64)
        inbox = np.full(len(pts), -1, np.int32)
        if len(boxes) and len(pts):
            big = enlarge(boxes, extra_width)
            hit = member(big, pts) & (box_labels >= 0)[:, None]
            inbox = np.where(hit.any(0), hit.argmax(0) + base, -1).astype(np.int32)
        fg = inbox >= 0
        local = np.clip(inbox - base, 0, None)
        lab = np.where(fg, box_labels[local] if len(boxes) else 0, bg_label).astype(np.int64)
        if len(boxes):
            if centers is not None:
                ctr = np.asarray(centers, F)[base:base + len(boxes)]
            else:
                ctr = np.stack([boxes[:, 0], boxes[:, 1], boxes[:, 2] + boxes[:, 5] * F(0.5)], 1).astype(F)
            delta = np.where(fg[:, None], ctr[local] - pts, F(0))
        else:
            delta = np.zeros_like(pts)
        labels.append(lab)
        targets.append(encode(delta))
        masks.append(fg)
        inboxes.append(inbox)
        base += len(boxes)
    return np.concatenate(labels), np.concatenate(targets), np.concatenate(masks), np.concatenate(inboxes)


def centroids64(points_list, boxes_list, inbox):
    """float64 mean of the member points of every box ([G_total, 3]; NaN for a box without points)"""
    pts = np.concatenate([np.asarray(p, np.float64)[:, :3] for p in points_list])
    g = sum(len(b) for b in boxes_list)
    out = np.full((g, 3), np.nan)
    for k in range(g):
        sel = inbox == k
        if sel.any():
            out[k] = pts[sel].mean(0)
    return out


def losses(logits, vote_preds, labels, vote_targets, vote_mask, mode, logit_scale=1.0, gamma=2.0, alpha=0.25,
           class_weight=None, score_thresh=None, class_group=None, dtype=torch.float64):
    """-> dict(loss_sem, loss_vote, num_valid, status, tp [C], real [C], recall [C], num_fg) - the formulas of
    include/sst_amd.h in ``dtype``; loss_sem and loss_vote are differentiable in logits / vote_preds."""
    n, c = logits.shape
    z = logits.to(dtype) * logit_scale
    labels = labels.long()
    mask = vote_mask.bool()
    is_class = (labels >= 0) & (labels < c)
    ok = is_class | (labels == c) if mode == SIGMOID_FOCAL else is_class
    status = (0 if bool(ok.all()) else 1) | (2 if bool((mask & ~is_class).any()) else 0)
    okf = ok.to(dtype)
    if mode == SIGMOID_FOCAL:
        t = ((labels[:, None] == torch.arange(c)[None]) & ok[:, None]).to(dtype)
        p = torch.sigmoid(z)
        # max(z, 0) - t z + log1p(exp(-|z|)), by torch's own function: autograd of the spelled-out formula takes one-sided
        # derivatives of max and |.| at z == 0 exactly (1 and 0) where the smooth function has sigmoid(0) - t
        bce = torch.nn.functional.binary_cross_entropy_with_logits(z, t, reduction='none')
        e = bce * (alpha * t + (1 - alpha) * (1 - t)) * (t - p).abs() ** gamma
        loss_sem = (e * okf[:, None]).sum() / (n * c)
    else:
        w = torch.ones(c, dtype=dtype) if class_weight is None else torch.as_tensor(class_weight, dtype=dtype)
        safe = labels.clamp(0, c - 1)
        e = -w[safe] * torch.log_softmax(z, 1).gather(1, safe[:, None])[:, 0]
        loss_sem = (e * okf).sum() / n
    voter = mask & is_class
    num_valid = int(voter.sum())
    if num_valid:
        safe = labels.clamp(0, c - 1)
        cols = (3 * safe)[:, None] + torch.arange(3)[None]
        picked = vote_preds.to(dtype).gather(1, cols)
        diff = (picked - vote_targets.to(dtype)).abs() * voter.to(dtype)[:, None]
        loss_vote = diff.sum() / (3 * num_valid)
    else:
        loss_vote = vote_preds.to(dtype).sum() * 0
    real = torch.stack([((labels == k) & ok).sum() for k in range(c)])
    tp = torch.zeros(c, dtype=torch.long)
    num_fg = 0
    margin = None   # distance of the nearest score from its threshold: the tests keep their inputs away from it
    if score_thresh is not None:
        with torch.no_grad():
            if mode == SIGMOID_FOCAL:
                thr = torch.as_tensor(score_thresh, dtype=dtype)
                score = torch.sigmoid(z)
                pred = score > thr[None]
                margin = float(((score - thr[None]).abs() + (~ok[:, None]).to(dtype)).min())
                tp = torch.stack([(pred[:, k] & (labels == k) & ok).sum() for k in range(c)])
            else:
                thr = torch.as_tensor(score_thresh, dtype=dtype)
                prob = torch.softmax(z, 1)[:, :-1]
                grp = torch.as_tensor(class_group)
                gs = torch.stack([prob[:, grp == g].sum(1) for g in range(len(thr))], 1)
                pred = (gs > thr[None]) & ok[:, None]
                margin = float(((gs - thr[None]).abs() + (~ok[:, None]).to(dtype)).min())
                num_fg = int(pred.sum())
                for k in range(c - 1):
                    if 0 <= int(grp[k]) < len(thr):
                        tp[k] = (pred[:, int(grp[k])] & (labels == k)).sum()
    recall = tp.to(torch.float32) / (real.to(torch.float32) + 1e-5)
    return dict(loss_sem=loss_sem, loss_vote=loss_vote, num_valid=num_valid, status=status, tp=tp, real=real, recall=recall,
                num_fg=num_fg, margin=margin)


def losses_and_grads(logits, vote_preds, labels, vote_targets, vote_mask, mode, w_sem=1.0, w_vote=1.0, **kw):
    """float64 run on CPU copies: the dict of ``losses`` (detached) plus d_logits / d_vote_preds of
    w_sem * loss_sem + w_vote * loss_vote"""
    lg = logits.detach().cpu().double().requires_grad_(True)
    vp = vote_preds.detach().cpu().double().requires_grad_(True)
    out = losses(lg, vp, labels.cpu(), vote_targets.detach().cpu(), vote_mask.cpu(), mode, **kw)
    (w_sem * out['loss_sem'] + w_vote * out['loss_vote']).backward()
    out['d_logits'] = lg.grad if lg.grad is not None else torch.zeros_like(lg)
    out['d_vote_preds'] = vp.grad if vp.grad is not None else torch.zeros_like(vp)
    out['loss_sem'], out['loss_vote'] = float(out['loss_sem'].detach()), float(out['loss_vote'].detach())
    return out
