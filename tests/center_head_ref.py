"""Restatement of what csrc/center_head.hip computes (include/sst_amd.h, "Training and decoding side of CenterHead"), for the
tests: the targets in numpy float32 with one rounded operation per step in the reference's order (np.sqrt is correctly
rounded; log / sin / cos / exp / atan2 are torch's CPU functions), the losses in torch with the dtype of the inputs (float64
for the tests' reference, gradients left to autograd), the decoding in float32.  Nothing here is used by the library."""
import numpy as np
import torch

from head_ref_common import ulp_distance  # noqa: F401  (the tests reach it through this module)

F = np.float32
HEAD_CHANNELS = (2, 1, 3, 2, 2)    # reg, height, dim, rot, vel


# ---- the cases of tests/golden/center_head_train.npz (tests/golden/make_center_head_train.py) ----------------------------------

W, H, CELL = 40, 36, 0.32
PC = [-W * CELL / 2, -H * CELL / 2, -2.0, W * CELL / 2, H * CELL / 2, 4.0]
NAMES = ['car', 'pedestrian', 'cyclist']
CODE_WEIGHTS = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2]
W_CLS, W_BBOX = 1.0, 2.0


def train_cfg(osf=1, max_objs=64):
    return dict(grid_size=[W * osf, H * osf, 1], voxel_size=(CELL / osf, CELL / osf, 6), out_size_factor=osf, dense_reg=1,
                gaussian_overlap=0.1, max_objs=max_objs, min_radius=2, point_cloud_range=PC, code_weights=CODE_WEIGHTS)


# name -> (train_cfg, tasks, norm_bbox, box columns)
CASES = {
    'shipped': (train_cfg(), [dict(num_class=3, class_names=NAMES)], True, 9),
    'osf2': (train_cfg(osf=2), [dict(num_class=3, class_names=NAMES)], False, 7),
    'two_tasks': (train_cfg(), [dict(num_class=2, class_names=NAMES[:2]), dict(num_class=1, class_names=NAMES[2:])], True, 9),
    'max8': (train_cfg(max_objs=8), [dict(num_class=3, class_names=NAMES)], True, 7),
}
LOSS_CASES = ('shipped', 'two_tasks')
DECODE_CASES = {'shipped': True, 'osf2': False}       # with the velocity head or without
MAX_NUM = 50
POST_CENTER_RANGE = [-5.01, -4.51, -2.53, 5.01, 4.51, 1.03]    # off the eighths the head maps lie on


def coder_cfg(case, score_threshold):
    cfg = CASES[case][0]
    return dict(pc_range=PC[:2], out_size_factor=cfg['out_size_factor'], voxel_size=list(cfg['voxel_size'][:2]),
                post_center_range=POST_CENTER_RANGE, max_num=MAX_NUM, score_threshold=score_threshold,
                code_size=9 if DECODE_CASES[case] else 7)


# ---- the restatement -----------------------------------------------------------------------------------------------

def task_table(tasks):
    out, first = [], 0
    for t in tasks:
        n = len(t['class_names'])
        out.append((first, n))
        first += n
    return out


def gaussian_radius(height, width, min_overlap):
    """gaussian.py:56-85 on float32 scalars; the Python scalars are formed in double and rounded to float32 once"""
    o = float(min_overlap)
    k_1m, k_1p, k_m2, k_16, k_m1 = F(1 - o), F(1 + o), F(-2 * o), F(4 * (4 * o)), F(o - 1)
    hw = F(height + width)
    b1 = hw
    c1 = F(F(F(width * height) * k_1m) / k_1p)
    sq1 = np.sqrt(F(F(b1 * b1) - F(F(4) * c1)))
    r1 = F(F(b1 + sq1) / F(2))
    b2 = F(F(2) * hw)
    c2 = F(F(k_1m * width) * height)
    sq2 = np.sqrt(F(F(b2 * b2) - F(F(16) * c2)))
    r2 = F(F(b2 + sq2) / F(2))
    b3 = F(k_m2 * hw)
    c3 = F(F(k_m1 * width) * height)
    sq3 = np.sqrt(F(F(b3 * b3) - F(k_16 * c3)))
    r3 = F(F(b3 + sq3) / F(2))
    return min(r1, r2, r3)


def _f32(fn, x):
    return fn(torch.from_numpy(np.ascontiguousarray(x, F))).numpy()


def targets(boxes_list, labels_list, tasks, cfg, norm_bbox):
    """-> (heatmaps, anno_boxes, inds, masks), per task batch-stacked numpy arrays"""
    table = task_table(tasks)
    osf = int(cfg['out_size_factor'])
    max_objs = int(cfg['max_objs']) * int(cfg.get('dense_reg', 1))
    w, h = int(cfg['grid_size'][0]) // osf, int(cfg['grid_size'][1]) // osf
    pc, vs = np.asarray(cfg['point_cloud_range'], F), np.asarray(cfg['voxel_size'], F)
    fo = F(osf)
    batch = len(boxes_list)
    out = ([], [], [], [])
    for first, count in table:
        hm = np.zeros((batch, count, h, w), F)
        anno = np.zeros((batch, max_objs, 10), F)
        ind = np.zeros((batch, max_objs), np.int64)
        mask = np.zeros((batch, max_objs), np.uint8)
        for s, (boxes, labels) in enumerate(zip(boxes_list, labels_list)):
            boxes, labels = np.asarray(boxes, F), np.asarray(labels, np.int64)
            order = [j for c in range(count) for j in np.nonzero(labels == first + c)[0]]
            if not len(boxes):
                continue
            logd = _f32(torch.log, boxes[:, 3:6])
            sin, cos = _f32(torch.sin, boxes[:, 6]), _f32(torch.cos, boxes[:, 6])
            for k, j in enumerate(order[:max_objs]):
                b = boxes[j]
                width, length = F(F(b[3] / vs[0]) / fo), F(F(b[4] / vs[1]) / fo)
                if not (width > 0 and length > 0):
                    continue
                radius = max(int(cfg['min_radius']), int(gaussian_radius(length, width, cfg['gaussian_overlap'])))
                cx, cy = F(F(F(b[0] - pc[0]) / vs[0]) / fo), F(F(F(b[1] - pc[1]) / vs[1]) / fo)
                x, y = int(cx), int(cy)    # truncation toward zero
                if not (0 <= x < w and 0 <= y < h):
                    continue
                left, right, top, bottom = min(x, radius), min(w - x, radius + 1), min(y, radius), min(h - y, radius + 1)
                sigma = (2 * radius + 1) / 6
                yy, xx = np.ogrid[-top:bottom, -left:right]
                g = np.exp(-(xx * xx + yy * yy).astype(np.float64) / (2 * sigma * sigma)).astype(F)
                patch = hm[s, labels[j] - first, y - top:y + bottom, x - left:x + right]
                np.maximum(patch, g, out=patch)
                ind[s, k], mask[s, k] = y * w + x, 1
                dims = logd[j] if norm_bbox else b[3:6]
                vel = b[7:9] if b.shape[0] >= 9 else np.zeros(2, F)
                anno[s, k] = np.concatenate([[F(cx - F(x)), F(cy - F(y)), F(b[2] + F(b[5] * F(0.5)))], dims, [sin[j], cos[j]], vel])
        for lst, a in zip(out, (hm, anno, ind, mask)):
            lst.append(a)
    return out


def gaussian_focal_terms(pred, target):
    """mmdet 2.x gaussian_focal_loss, alpha 2, gamma 4, per cell"""
    eps = 1e-12
    pos = -(pred + eps).log() * (1 - pred).pow(2) * target.eq(1).to(pred.dtype)
    neg = -(1 - pred + eps).log() * pred.pow(2) * (1 - target).pow(4)
    return pos + neg


def losses(logits, heads, heatmap, anno, ind, mask, code_weights, w_cls, w_bbox):
    """-> (loss_heatmap, loss_bbox) in the dtype of ``logits``; heads: the present NCHW maps in order"""
    dt = logits.dtype
    heatmap = heatmap.to(dt)
    p = torch.clamp(logits.sigmoid(), min=1e-4, max=1 - 1e-4)
    num_pos = heatmap.eq(1).to(dt).sum()
    loss_hm = gaussian_focal_terms(p, heatmap).sum() / torch.clamp(num_pos, min=1) * w_cls
    pred = torch.cat(list(heads), 1)
    b, c = pred.shape[:2]
    pred = pred.permute(0, 2, 3, 1).reshape(b, -1, c)
    pred = pred.gather(1, ind.unsqueeze(2).expand(-1, -1, c))
    m = mask.to(dt)
    # the reference forms the weights and avg_factor = mask.float().sum() + 1e-4 in float32 whatever the dtype of the predictions
    weights = m.unsqueeze(2) * torch.as_tensor(code_weights, dtype=torch.float32)[:c].to(dt)
    avg = (mask.float().sum() + 1e-4).to(dt)
    loss_box = ((pred - anno.to(dt)[..., :c]).abs() * weights).sum() / avg * w_bbox
    return loss_hm, loss_box


def losses_and_grads(logits, heads, heatmap, anno, ind, mask, code_weights, w_cls, w_bbox, dtype=torch.float64):
    """numpy in -> dict(loss_heatmap, loss_bbox, d_logits, d_heads (list)) by autograd in ``dtype``"""
    lg = torch.as_tensor(logits).to(dtype).requires_grad_(True)
    hs = [torch.as_tensor(h).to(dtype).requires_grad_(True) for h in heads]
    l_hm, l_box = losses(lg, hs, torch.as_tensor(heatmap), torch.as_tensor(anno), torch.as_tensor(ind).long(),
                         torch.as_tensor(mask), code_weights, w_cls, w_bbox)
    (l_hm + l_box).backward()
    return dict(loss_heatmap=l_hm.detach().numpy(), loss_bbox=l_box.detach().numpy(), d_logits=lg.grad.numpy(),
                d_heads=[(h.grad if h.grad is not None else torch.zeros_like(h)).numpy() for h in hs])


def split_heads(maps, with_vel=True):
    """[B, 10, H, W] -> reg, height, dim, rot (, vel)"""
    out, at = [], 0
    for c in HEAD_CHANNELS[:5 if with_vel else 4]:
        out.append(np.ascontiguousarray(maps[:, at:at + c]))
        at += c
    return out


def heat_of(logits):
    """the decode cases' scores: exact float32 arithmetic only (a power-of-two scale, one rounded addition), so every machine
    forms the same bits"""
    return np.clip(np.asarray(logits, F) * F(1 / 32) + F(0.5), F(0), F(1)).astype(F)


def decode(heat, reg, hei, dim, rot, vel, coder, norm_bbox):
    """-> (boxes [B, K, 9 / 7], scores, labels int [B, K], keep bool) in float32, the coder's operation order"""
    heat = torch.from_numpy(np.ascontiguousarray(heat, F))
    b, c, h, w = heat.shape
    k = int(coder['max_num'])
    s1, i1 = torch.topk(heat.reshape(b, c, -1), k)
    i1 = i1 % (h * w)
    scores, i2 = torch.topk(s1.view(b, -1), k)
    labels = (i2 / torch.tensor(k, dtype=torch.float)).int().numpy()
    inds = i1.view(b, -1).gather(1, i2).numpy()
    scores = scores.numpy()
    ys0 = (inds.astype(F) / F(w)).astype(np.int32).astype(F)
    xs0 = (inds % w).astype(F)

    def at(m, ch):
        flat = np.asarray(m, F).reshape(b, m.shape[1], -1)
        return np.take_along_axis(flat[:, ch], inds, 1)

    osf, vs, pc = F(coder['out_size_factor']), np.asarray(coder['voxel_size'], F), np.asarray(coder['pc_range'], F)
    rx, ry = (at(reg, 0), at(reg, 1)) if reg is not None else (F(0.5), F(0.5))
    x = F(F(F(xs0 + rx) * osf) * vs[0]) + pc[0]
    y = F(F(F(ys0 + ry) * osf) * vs[1]) + pc[1]
    z = at(hei, 0)
    dims = [at(dim, i) for i in range(3)]
    if norm_bbox:
        dims = [_f32(torch.exp, d) for d in dims]
    ang = torch.atan2(torch.from_numpy(at(rot, 0)), torch.from_numpy(at(rot, 1))).numpy()
    cols = [x, y, z] + dims + [ang] + ([at(vel, 0), at(vel, 1)] if vel is not None else [])
    boxes = np.stack(cols, 2).astype(F)
    keep = np.ones_like(scores, bool)
    if coder.get('score_threshold'):
        keep &= scores > F(coder['score_threshold'])
    r = np.asarray(coder['post_center_range'], F)
    keep &= (boxes[..., :3] >= r[:3]).all(2) & (boxes[..., :3] <= r[3:]).all(2)
    return boxes, scores, labels, keep
