"""Host restatements of the rotated-box ops (csrc/box_ops.hip), for tests/test_box_ops_host.py and
tests/test_gpu_box_ops.py.

- bev_overlap_f32 / bev_iou_f32: the reference's polygon algorithm (ops/iou3d/src/iou3d_kernel.cu:54-251) in numpy
  float32, vectorised over pairs: the same operations in the same order, one rounding per product and sum.  The
  intersection points and the corners inside the other box take fixed slots in the reference's order of appending;
  a stable sort of the angles with +inf for empty slots then yields exactly the reference's compacted, bubble-sorted
  list.
- bev_overlap_f64: an independent float64 polygon clip (Sutherland-Hodgman) with the same corner convention.
- nms_host: the reference's greedy sweep (iou3d.cpp:116-133) over a float32 IoU, using only the pairs whose
  circumscribed circles meet (every other pair has IoU 0 exactly).
- multiclass_nms_host: core/post_processing/box3d_nms.py:10-143 with that NMS.
"""
import numpy as np

F32 = np.float32
EPS = F32(1e-8)
MARGIN = F32(1e-5)
CAP = 16

# Largest |float32 restatement - float64 clip| of the BEV IoU over random_pairs(2500, 0) (test_box_ops_host.py):
# 3.0e-6 measured, rounded up; the GPU kernel is held to the same bar against float64.
F32_IOU_NOISE = 1e-5


def random_pairs(n, seed):
    """centres within +-75 m, sizes 0.3 - 20 m, any angle; box b is placed near box a so that most pairs overlap"""
    rng = np.random.default_rng(seed)
    ca = rng.uniform(-75, 75, (n, 2))
    sa, sb = rng.uniform(0.3, 20, (n, 2)), rng.uniform(0.3, 20, (n, 2))
    cb = ca + rng.uniform(-1, 1, (n, 2)) * (sa + sb) / 2
    ra, rb = rng.uniform(-np.pi, np.pi, n), rng.uniform(-np.pi, np.pi, n)
    a = np.column_stack([ca - sa / 2, ca + sa / 2, ra]).astype(F32)
    b = np.column_stack([cb - sb / 2, cb + sb / 2, rb]).astype(F32)
    return a, b


def _rot(cx, cy, cs, sn, x, y):
    dx, dy = x - cx, y - cy
    return dx * cs + dy * sn + cx, -dx * sn + dy * cs + cy


def _cross3(p1x, p1y, p2x, p2y, p0x, p0y):
    return (p1x - p0x) * (p2y - p0y) - (p2x - p0x) * (p1y - p0y)


def _edge_cross(p1, p0, q1, q0):
    (p1x, p1y), (p0x, p0y), (q1x, q1y), (q0x, q0y) = p1, p0, q1, q0
    ok = ((np.minimum(p0x, p1x) <= np.maximum(q0x, q1x)) & (np.minimum(q0x, q1x) <= np.maximum(p0x, p1x)) &
          (np.minimum(p0y, p1y) <= np.maximum(q0y, q1y)) & (np.minimum(q0y, q1y) <= np.maximum(p0y, p1y)))
    s1 = _cross3(q0x, q0y, p1x, p1y, p0x, p0y)
    s2 = _cross3(p1x, p1y, q1x, q1y, p0x, p0y)
    s3 = _cross3(p0x, p0y, q1x, q1y, q0x, q0y)
    s4 = _cross3(q1x, q1y, p1x, p1y, q0x, q0y)
    ok &= (s1 * s2 > 0) & (s3 * s4 > 0)
    s5 = _cross3(q1x, q1y, p1x, p1y, p0x, p0y)
    d = s5 - s1
    x_a = (s5 * q0x - s1 * q1x) / d
    y_a = (s5 * q0y - s1 * q1y) / d
    a0, b0, c0 = p0y - p1y, p1x - p0x, p0x * p1y - p1x * p0y
    a1, b1, c1 = q0y - q1y, q1x - q0x, q0x * q1y - q1x * q0y
    dd = a0 * b1 - a1 * b0
    x_b = (b0 * c1 - b1 * c0) / dd
    y_b = (a1 * c0 - a0 * c1) / dd
    main = np.abs(d) > EPS
    return ok, np.where(main, x_a, x_b), np.where(main, y_a, y_b)


def _corners(b, cx, cy):
    cs, sn = np.cos(b[:, 4]), np.sin(b[:, 4])
    xs = (b[:, 0], b[:, 2], b[:, 2], b[:, 0])
    ys = (b[:, 1], b[:, 1], b[:, 3], b[:, 3])
    pts = [_rot(cx, cy, cs, sn, x, y) for x, y in zip(xs, ys)]
    return pts + [pts[0]]


def _in_box(b, cx, cy, p):
    cs, sn = np.cos(-b[:, 4]), np.sin(-b[:, 4])
    rx, ry = _rot(cx, cy, cs, sn, p[0], p[1])
    return (rx > b[:, 0] - MARGIN) & (rx < b[:, 2] + MARGIN) & (ry > b[:, 1] - MARGIN) & (ry < b[:, 3] + MARGIN)


def bev_overlap_f32(a, b):
    """overlap areas of pairs (a[i], b[i]); a, b [N, 5] ([x1, y1, x2, y2, ry]) -> [N] float32"""
    a = np.ascontiguousarray(a, dtype=F32).reshape(-1, 5)
    b = np.ascontiguousarray(b, dtype=F32).reshape(-1, 5)
    n = a.shape[0]
    with np.errstate(all='ignore'):
        cax, cay = (a[:, 0] + a[:, 2]) / F32(2), (a[:, 1] + a[:, 3]) / F32(2)
        cbx, cby = (b[:, 0] + b[:, 2]) / F32(2), (b[:, 1] + b[:, 3]) / F32(2)
        pa, pb = _corners(a, cax, cay), _corners(b, cbx, cby)
        sx, sy, sv = [], [], []
        for i in range(4):
            for j in range(4):
                ok, x, y = _edge_cross(pa[i + 1], pa[i], pb[j + 1], pb[j])
                sx.append(x), sy.append(y), sv.append(ok)
        for k in range(4):
            sx.append(pb[k][0]), sy.append(pb[k][1]), sv.append(_in_box(a, cax, cay, pb[k]))
            sx.append(pa[k][0]), sy.append(pa[k][1]), sv.append(_in_box(b, cbx, cby, pa[k]))
        sx, sy, sv = np.stack(sx, 1), np.stack(sy, 1), np.stack(sv, 1)
        sv &= np.cumsum(sv, 1) <= CAP  # the kernel keeps the first CAP points, as the reference's cross_points[16]
        cnt = sv.sum(1)
        ctx, cty = np.zeros(n, F32), np.zeros(n, F32)
        for s in range(sx.shape[1]):
            ctx = np.where(sv[:, s], ctx + sx[:, s], ctx)
            cty = np.where(sv[:, s], cty + sy[:, s], cty)
        ctx = ctx / cnt.astype(F32)
        cty = cty / cnt.astype(F32)
        key = np.where(sv, np.arctan2(sy - cty[:, None], sx - ctx[:, None]), F32(np.inf))
        order = np.argsort(key, axis=1, kind='stable')
        px = np.take_along_axis(sx, order, 1)
        py = np.take_along_axis(sy, order, 1)
        area = np.zeros(n, F32)
        ux, uy = px[:, 1] - px[:, 0], py[:, 1] - py[:, 0]
        for k in range(1, CAP - 1):
            vx, vy = px[:, k + 1] - px[:, 0], py[:, k + 1] - py[:, 0]
            area = np.where(k < cnt - 1, area + (ux * vy - uy * vx), area)
            ux, uy = vx, vy
        out = np.where(cnt >= 3, np.abs(area) / F32(2), F32(0))
    return out.astype(F32)


def bev_iou_f32(a, b):
    a = np.asarray(a, F32).reshape(-1, 5)
    b = np.asarray(b, F32).reshape(-1, 5)
    s = bev_overlap_f32(a, b)
    sa = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    sb = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return (s / np.maximum(sa + sb - s, EPS)).astype(F32)


def axis_iou_f32(a, b):
    a = np.asarray(a, F32).reshape(-1, 5)
    b = np.asarray(b, F32).reshape(-1, 5)
    w = np.maximum(np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0]), F32(0))
    h = np.maximum(np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1]), F32(0))
    inter = w * h
    sa = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    sb = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return (inter / np.maximum(sa + sb - inter, EPS)).astype(F32)


def pairwise(fn, a, b):
    a = np.asarray(a, F32).reshape(-1, 5)
    b = np.asarray(b, F32).reshape(-1, 5)
    ia, ib = np.meshgrid(np.arange(len(a)), np.arange(len(b)), indexing='ij')
    return fn(a[ia.ravel()], b[ib.ravel()]).reshape(len(a), len(b))


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference geometry
# ---------------------------------------------------------------------------------------------------------------------
def _poly64(box):
    x1, y1, x2, y2, r = (float(v) for v in box)
    cx, cy = (x1 + x2) / 2, (y1 + y2) / 2
    c, s = np.cos(r), np.sin(r)
    out = []
    for x, y in ((x1, y1), (x2, y1), (x2, y2), (x1, y2)):
        dx, dy = x - cx, y - cy
        out.append((dx * c + dy * s + cx, -dx * s + dy * c + cy))  # the kernel's rotation convention
    return out


def _area64(poly):
    return 0.5 * abs(sum(poly[i][0] * poly[(i + 1) % len(poly)][1] - poly[(i + 1) % len(poly)][0] * poly[i][1]
                         for i in range(len(poly))))


def bev_overlap_f64(a, b):
    """Sutherland-Hodgman clip of box a by box b (both convex, counter-clockwise), float64"""
    subject, clip = _poly64(a), _poly64(b)
    for i in range(4):
        (ex0, ey0), (ex1, ey1) = clip[i], clip[(i + 1) % 4]

        def side(p):
            return (ex1 - ex0) * (p[1] - ey0) - (ey1 - ey0) * (p[0] - ex0)

        inp, subject = subject, []
        for k in range(len(inp)):
            cur, prev = inp[k], inp[k - 1]
            sc, sp = side(cur), side(prev)
            if sc >= 0:
                if sp < 0:
                    t = sp / (sp - sc)
                    subject.append((prev[0] + t * (cur[0] - prev[0]), prev[1] + t * (cur[1] - prev[1])))
                subject.append(cur)
            elif sp >= 0:
                t = sp / (sp - sc)
                subject.append((prev[0] + t * (cur[0] - prev[0]), prev[1] + t * (cur[1] - prev[1])))
        if not subject:
            return 0.0
    return _area64(subject) if len(subject) >= 3 else 0.0


def bev_iou_f64(a, b):
    s = bev_overlap_f64(a, b)
    sa = (float(a[2]) - float(a[0])) * (float(a[3]) - float(a[1]))
    sb = (float(b[2]) - float(b[0])) * (float(b[3]) - float(b[1]))
    return s / max(sa + sb - s, 1e-8)


# ---------------------------------------------------------------------------------------------------------------------
# NMS and multi-class NMS
# ---------------------------------------------------------------------------------------------------------------------
def near_pairs(boxes):
    """pairs (i < j) whose circumscribed circles meet (with a 2 cm slack); every other pair has overlap 0"""
    b = np.asarray(boxes, np.float64).reshape(-1, 5)
    cx, cy = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
    r = 0.5 * np.hypot(b[:, 2] - b[:, 0], b[:, 3] - b[:, 1])
    ii, jj = [], []
    step = 2048
    for s in range(0, len(b), step):
        d2 = (cx[s:s + step, None] - cx[None]) ** 2 + (cy[s:s + step, None] - cy[None]) ** 2
        reach = (r[s:s + step, None] + r[None]) * 1.002 + 2e-2
        i, j = np.nonzero(d2 <= reach * reach)
        i = i + s
        m = j > i
        ii.append(i[m]), jj.append(j[m])
    return (np.concatenate(ii) if ii else np.zeros(0, np.int64)), (np.concatenate(jj) if jj else np.zeros(0, np.int64))


def nms_host(sorted_boxes, thresh, rotated=True, groups=None, group_thresh=None, pairs=None):
    """the reference's greedy sweep over boxes sorted by descending score -> kept positions"""
    b = np.asarray(sorted_boxes, F32).reshape(-1, 5)
    n = len(b)
    # the circumscribed circle of a box also holds its axis-aligned form: pairs apart have IoU 0 in both modes
    ii, jj = near_pairs(b) if pairs is None else pairs
    ii, jj = np.asarray(ii), np.asarray(jj)
    iou = (bev_iou_f32 if rotated else axis_iou_f32)(b[ii], b[jj]) if len(ii) else np.zeros(0, F32)
    if groups is None:
        thr = np.full(len(ii), F32(thresh))
        same = np.ones(len(ii), bool)
    else:
        g = np.asarray(groups)
        gt = np.array([np.inf if t is None else t for t in group_thresh], F32)
        same = g[ii] == g[jj]
        thr = gt[g[ii]]
    sup = same & (iou > thr)
    succ = [[] for _ in range(n)]
    for i, j in zip(ii[sup], jj[sup]):
        succ[i].append(j)
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if not removed[i]:
            keep.append(i)
            removed[succ[i]] = True
    return np.array(keep, np.int64)


def multiclass_nms_host(bboxes, bboxes_for_nms, scores, score_thr, max_num, nms_thr, rotated,
                        dir_scores=None, attr_scores=None, bboxes2d=None):
    """core/post_processing/box3d_nms.py:10-143 over numpy arrays, NMS by nms_host (scores distinct per class)"""
    num_classes = scores.shape[1] - 1
    out = {k: [] for k in ('bboxes', 'scores', 'labels', 'dir', 'attr', 'b2d')}
    for i in range(num_classes):
        st = score_thr[i] if isinstance(score_thr, (list, tuple)) else score_thr
        nt = nms_thr[i] if isinstance(nms_thr, (list, tuple)) else nms_thr
        inds = np.nonzero(scores[:, i] > F32(st))[0]
        if len(inds) == 0:
            continue
        s = scores[inds, i]
        if nt is None:
            sel = np.arange(len(inds))
        else:
            order = np.argsort(-s, kind='stable')
            sel = order[nms_host(bboxes_for_nms[inds][order], nt, rotated)]
        out['bboxes'].append(bboxes[inds][sel])
        out['scores'].append(s[sel])
        out['labels'].append(np.full(len(sel), i, np.int64))
        for k, v in (('dir', dir_scores), ('attr', attr_scores), ('b2d', bboxes2d)):
            if v is not None:
                out[k].append(v[inds][sel])
    if not out['bboxes']:
        return None
    res = {k: np.concatenate(v) for k, v in out.items() if v}
    if len(res['bboxes']) > max_num:
        inds = np.argsort(-res['scores'], kind='stable')[:max_num]
        res = {k: v[inds] for k, v in res.items()}
    return res
