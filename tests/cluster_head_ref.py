"""Restatement of what csrc/cluster_head.hip computes (include/sst_amd.h, "Training and decoding side of the FSD cluster
heads"), for the tests: torch on the CPU in float32 or float64, in the FUSED data flow - one pass over the concatenated boxes
for all tasks, no split by sample, no regrouping of the ground truth - with the gradients left to autograd.  Nothing here is
used by the library."""
import numpy as np
import torch

import box_ops_ref as B
import seg_loss_ref as S

F = np.float32
ulp_distance = S.ulp_distance

WAYMO_NAMES = ['Car', 'Pedestrian', 'Cyclist']
WAYMO_TASKS = [dict(class_names=['Car']), dict(class_names=['Pedestrian']), dict(class_names=['Cyclist'])]
# two multi-class tasks whose class order differs from the order of the class indices (FSDV2Head only asks that the names match)
MULTI_NAMES = ['car', 'truck', 'bus', 'bicycle', 'pedestrian', 'cone']
MULTI_TASKS = [dict(class_names=['bus', 'car', 'truck']), dict(class_names=['pedestrian', 'cone', 'bicycle'])]
WIDTHS = {'none': None, 'p03': 0.3, 'm02': -0.2}
LOSS_CFG = dict(gamma=2.0, alpha=0.25, w_cls=2.0, w_center=0.5, w_size=0.5, w_rot=0.2, w_vel=0.2)
LOSS_CASES = ('waymo_none', 'multi_none', 'multi_centroid')   # the cases whose gradients the golden file holds
CODE_WEIGHT10 = [1.0, 1.0, 0.5, 1.0, 2.0, 1.0, 0.25, 1.0, 0.2, 0.2]


def class_table(tasks, class_names):
    """[(task, class index within the task)] per global class; (-1, 0) for a class in no task"""
    table = [(-1, 0)] * len(class_names)
    for t, task in enumerate(tasks):
        for i, name in enumerate(task['class_names']):
            table[class_names.index(name)] = (t, i)
    return table


def enlarge(boxes, width):
    """enlarged_box (lidar_box3d.py:269-285) on [G, >= 7] float32: w, l, h += (float)(2 width), z -= (float)width; for a negative
    width a box whose enlarged w, l or h would be <= 0 keeps its own extents"""
    boxes = np.asarray(boxes, F)[:, :7]
    out = boxes.copy()
    if width is None:
        return out
    out[:, 3:6] = out[:, 3:6] + F(width * 2)
    out[:, 2] = out[:, 2] - F(width)
    if width < 0:
        bad = (out[:, 3:6] <= 0).any(1)
        out[bad] = boxes[bad]
    return out


def near_a_face(boxes, pts, tol=1e-3):
    """float64: points within tol of a face plane of any box, at its own size or enlarged by any of WIDTHS"""
    boxes = np.asarray(boxes, np.float64)[:, :7]
    bad = np.zeros(len(pts), bool)
    for w in WIDTHS.values():
        b = boxes.copy()
        if w is not None:
            b[:, 3:6] += 2 * w
            b[:, 2] -= w
            inv = (b[:, 3:6] <= 0).any(1)
            b[inv] = boxes[inv]
        bad |= S.near_a_face(b, pts, widths=(), tol=tol)
    return bad


def targets(xyz_assign, xyz_base, batch_idx, boxes_list, labels_list, tasks, class_names, code, width=None, dtype=torch.float32):
    """-> per task (labels int64 [N], assigned int64 [N] into the concatenated boxes or -1, bbox_targets [N, code], bbox_weights
    [N, code]) as torch tensors of ``dtype``.  Membership is decided in float32 (csrc/pib_test.h restated by
    seg_loss_ref.inside); the scenes of the tests keep every point 1e-3 away from every face."""
    xa = np.asarray(xyz_assign, F)
    n = len(xa)
    bidx = np.asarray(batch_idx, np.int64)
    base = torch.as_tensor(np.asarray(xyz_base)).to(dtype)
    cols = max([np.asarray(b).shape[1] for b in boxes_list if len(b)] or [7 if code == 8 else 9])
    boxes = np.concatenate([np.asarray(b, F).reshape(-1, cols) for b in boxes_list]) if boxes_list else np.zeros((0, cols), F)
    labels = np.concatenate([np.asarray(l, np.int64).reshape(-1) for l in labels_list])
    sample_of_box = np.concatenate([np.full(len(l), s, np.int64) for s, l in enumerate(labels_list)])
    table = class_table(tasks, class_names)
    g = len(boxes)
    hit = np.zeros((g, n), bool)
    if g and n:
        hit = S.inside(enlarge(boxes, width), xa) & (sample_of_box[:, None] == bidx[None, :])
    tboxes = torch.as_tensor(boxes).to(dtype)
    out = []
    for t, task in enumerate(tasks):
        c = len(task['class_names'])
        in_task = np.array([0 <= l < len(table) and table[l][0] == t for l in labels], bool)
        idx_in_task = np.array([table[l][1] if 0 <= l < len(table) else 0 for l in labels], np.int64)
        # the smallest (class index within the task, box index) among the hits
        key = np.where(in_task, idx_in_task * (g + 1) + np.arange(g), np.iinfo(np.int64).max)
        keyed = np.where(hit & in_task[:, None], key[:, None], np.iinfo(np.int64).max)
        best = keyed.min(0) if g else np.full(n, np.iinfo(np.int64).max)
        pos = best != np.iinfo(np.int64).max
        assigned = np.where(pos, best % (g + 1), -1).astype(np.int64)
        lab = np.where(pos, best // (g + 1), c).astype(np.int64)
        tg = torch.zeros((n, code), dtype=dtype)
        wt = torch.zeros((n, code), dtype=dtype)
        if pos.any():
            rows = torch.as_tensor(np.nonzero(pos)[0])
            bx = tboxes[torch.as_tensor(assigned[pos])]
            eps = torch.tensor(1e-6, dtype=dtype)
            enc = [bx[:, :3] - base[rows], (bx[:, 3:6] + eps).log(), bx[:, 6:7].sin(), bx[:, 6:7].cos()]
            if code == 10:
                enc.append(bx[:, 7:9])
            tg[rows] = torch.cat(enc, 1)
            wt[rows] = 1.0
            if cols == 10:
                wt[rows, code - 2:] = bx[:, 9:10].expand(-1, 2)
        out.append((torch.as_tensor(lab), torch.as_tensor(assigned), tg, wt))
    return out


GROUPS = ((0, 3), (3, 6), (6, 8), (8, 10))
LOSS_NAMES = ('loss_cls', 'loss_center', 'loss_size', 'loss_rot', 'loss_vel')


def task_losses(logits, reg, labels, tg, wt, cfg=LOSS_CFG, code_weight=None, cls_avg=None, reg_avg=None, beta=None,
                dtype=torch.float64):
    """-> dict(loss_cls, loss_center, loss_size, loss_rot, loss_vel, num_pos, status) of one task in ``dtype``"""
    n, c = logits.shape
    code = reg.shape[1]
    z = logits.to(dtype)
    pos = (labels >= 0) & (labels < c)
    ok = pos | (labels == c)
    t = ((labels[:, None] == torch.arange(c)[None]) & ok[:, None]).to(dtype)
    p = torch.sigmoid(z)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(z, t, reduction='none')
    e = bce * (cfg['alpha'] * t + (1 - cfg['alpha']) * (1 - t)) * (t - p).abs() ** cfg['gamma']
    num_pos = int(pos.sum())
    cls_avg = float(n) if cls_avg is None else cls_avg
    reg_avg = float(num_pos) if reg_avg is None else reg_avg
    out = dict(loss_cls=cfg['w_cls'] * (e * ok.to(dtype)[:, None]).sum() / cls_avg, num_pos=num_pos)
    w = wt.to(dtype)
    if code_weight:
        w = w * torch.as_tensor(code_weight, dtype=dtype)[None, :code]
    diff = (reg.to(dtype) - tg.to(dtype)).abs()
    if beta:      # mmdet's smooth_l1_loss per loss (beta[k] in the order of LOSS_NAMES, 0: L1)
        b = torch.tensor([beta[1]] * 3 + [beta[2]] * 3 + [beta[3]] * 2 + [beta[4]] * 2, dtype=dtype)[None, :code]
        diff = torch.where(diff < b, 0.5 * diff * diff / b.clamp(min=1e-30), diff - 0.5 * b)
    diff = diff * w * pos.to(dtype)[:, None]
    for name, (lo, hi) in zip(LOSS_NAMES[1:], GROUPS):
        if lo >= code:
            continue
        if num_pos == 0:
            out[name] = reg.to(dtype).sum() * 0
        elif name == 'loss_vel':
            out[name] = cfg['w_vel'] * diff[:, lo:hi].sum() / (2 * num_pos)
        else:
            out[name] = cfg['w_' + name[5:]] * diff[:, lo:hi].sum() / reg_avg
    bad_flag = code == 10 and bool(((wt[:, 8:] != 0) & (wt[:, 8:] != 1) & pos[:, None]).any())
    out['status'] = (0 if bool(ok.all()) else 1) | (2 if bad_flag else 0)
    return out


def losses_and_grads(logits, reg, labels, tg, wt, upstream=None, **kw):
    """float64 run on CPU copies: the losses as floats plus d_logits / d_reg of sum_k upstream[k] * loss_k"""
    lg = torch.as_tensor(np.asarray(logits)).double().requires_grad_(True)
    rp = torch.as_tensor(np.asarray(reg)).double().requires_grad_(True)
    out = task_losses(lg, rp, torch.as_tensor(np.asarray(labels)), torch.as_tensor(np.asarray(tg)),
                      torch.as_tensor(np.asarray(wt)), **kw)
    names = [k for k in LOSS_NAMES if k in out]
    up = upstream or [1.0] * 5
    total = sum(up[LOSS_NAMES.index(k)] * out[k] for k in names)
    total.backward()
    res = {k: float(out[k].detach()) for k in names}
    res.update(num_pos=out['num_pos'], status=out['status'])
    res['d_logits'] = lg.grad if lg.grad is not None else torch.zeros_like(lg)
    res['d_reg'] = rp.grad if rp.grad is not None else torch.zeros_like(rp)
    return res


def decode(reg, base, logits=None, dtype=torch.float32):
    """BasePointBBoxCoder.decode, the padded sigmoid scores and the (x1, y1, x2, y2, r) rows of the NMS"""
    reg = torch.as_tensor(np.asarray(reg)).to(dtype)
    base = torch.as_tensor(np.asarray(base)).to(dtype)
    eps = torch.tensor(1e-6, dtype=dtype)
    parts = [reg[:, :3] + base, reg[:, 3:6].exp() - eps, torch.atan2(reg[:, 6:7], reg[:, 7:8])]
    if reg.shape[1] == 10:
        parts.append(reg[:, 8:10])
    boxes = torch.cat(parts, 1)
    half_w, half_l = boxes[:, 3] / 2, boxes[:, 4] / 2
    bev = torch.stack([boxes[:, 0] - half_w, boxes[:, 1] - half_l, boxes[:, 0] + half_w, boxes[:, 1] + half_l, boxes[:, 6]], 1)
    scores = None
    if logits is not None:
        s = torch.as_tensor(np.asarray(logits)).to(dtype).sigmoid()
        scores = torch.cat([s, s.new_zeros((len(s), 1))], 1)
    return boxes, scores, bev


def get_bboxes(cls_logits, reg_preds, xyz, batch_idx, batch, tasks, class_names, cfg, all_task_max_num=None):
    """_get_bboxes_single per (task, sample) on the restated decode with the NMS of box_ops_ref -> per sample (boxes, scores,
    labels) as numpy"""
    bidx = np.asarray(batch_idx, np.int64)
    per_sample = [[] for _ in range(batch)]
    for t, task in enumerate(tasks):
        boxes, scores, bev = (v.numpy() for v in decode(reg_preds[t], xyz, cls_logits[t]))
        for s in range(batch):
            sel = np.nonzero(bidx == s)[0]
            nms_pre = cfg.get('nms_pre', -1)
            if nms_pre > 0 and len(sel) > nms_pre:
                top = np.argsort(-scores[sel, :-1].max(1), kind='stable')[:nms_pre]
                sel = sel[top]
            res = B.multiclass_nms_host(boxes[sel], bev[sel], scores[sel], cfg.get('score_thr', 0), cfg['max_num'],
                                        cfg['nms_thr'], cfg['use_rotate_nms']) if len(sel) else None
            if res is None:
                per_sample[s].append((np.zeros((0, boxes.shape[1]), F), np.zeros(0, F), np.zeros(0, np.int64)))
                continue
            glob = np.array([class_names.index(task['class_names'][i]) for i in res['labels']], np.int64)
            per_sample[s].append((res['bboxes'], res['scores'], glob))
    out = []
    for s in range(batch):
        b, sc, lb = (np.concatenate([r[k] for r in per_sample[s]]) for k in range(3))
        if all_task_max_num is not None and len(sc) > all_task_max_num:
            top = np.argsort(-sc, kind='stable')[:all_task_max_num]
            b, sc, lb = b[top], sc[top], lb[top]
        out.append((b, sc, lb))
    return out
