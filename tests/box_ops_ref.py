"""Host restatements of the rotated-box ops (csrc/box_ops.hip), for tests/test_box_ops_host.py,
tests/test_gpu_box_ops.py, tests/test_box_ops_detector_host.py and tests/test_gpu_box_ops_detector.py.

- bev_overlap_f32 / bev_iou_f32: the reference's polygon algorithm (ops/iou3d/src/iou3d_kernel.cu:54-251) in numpy
  float32, vectorised over pairs: the same operations in the same order, one rounding per product and sum.  The
  intersection points and the corners inside the other box take fixed slots in the reference's order of appending;
  a stable sort of the angles with +inf for empty slots then yields exactly the reference's compacted, bubble-sorted
  list.
- bev_overlap_f64: an independent float64 polygon clip (Sutherland-Hodgman) with the same corner convention.
- nms_host: the reference's greedy sweep (iou3d.cpp:116-133) over a float32 IoU, using only the pairs whose
  circumscribed circles meet (every other pair has IoU 0 exactly).
- multiclass_nms_host: core/post_processing/box3d_nms.py:10-143 with that NMS.
- detector_pairs / detector_boxes / detector_nms_inputs: inputs as a detection head emits them, with the noise bounds
  measured on them (DETECTOR_IOU_NOISE, DETECTOR_AREA_NOISE); chain_boxes / periodic_boxes / dense_boxes: NMS inputs
  with exact IoUs and analytic keep lists.
"""
import functools

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


def cluster_boxes(n, seed, extent=75.0):
    """boxes scattered uniformly within +-extent, sizes 0.5 - 6 m, any angle"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-extent, extent, (n, 2))
    s = rng.uniform(0.5, 6.0, (n, 2))
    return np.column_stack([c - s / 2, c + s / 2, rng.uniform(-np.pi, np.pi, n)]).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# detector-like inputs: clusters of near-duplicate boxes, as a detection head emits them
# ---------------------------------------------------------------------------------------------------------------------
DETECTOR_FAMILIES = ('jitter', 'same_angle', 'quarter_turn', 'tiny_angle', 'shift_only', 'axis0', 'big_angle',
                     'identical')
DETECTOR_SEED = 1  # the seed of every measurement below and of the tests that use the bounds

# A pair is UNSTABLE when the float32 restatement is more than this from the float64 clip: the reference's polygon
# algorithm itself lost or doubled a polygon point there (a corner on the 1e-5 in-box margin, a crossing of two
# near-parallel edges), and one ulp in a sine decides on which side it lands.  No |1 - IoU| between 1e-4 and 1e-1 was
# found over 36 000 identical-box pairs, so the cut separates the two populations.  Unstable pairs are excused, and
# their share is bounded (UNSTABLE_SHARE_MAX): measured 0 for seven families and 0.95 % for `identical` (the reference's
# algorithm returns IoU < 0.5 for 19 of 2000 identical boxes with centres within +-75 m at seed 1, 16 of 2000 at seed
# 2, 94 of 20 000 at seed 3; parity with the reference is the contract, so this is documented and not repaired).
UNSTABLE_GAP = 1e-3
UNSTABLE_SHARE_MAX = 0.02

# Largest |float32 restatement - float64 clip| of the BEV IoU over the STABLE pairs of detector_pairs(family, 2000,
# DETECTOR_SEED), all eight families, measured on the CPU (numpy float32; the kernel is not involved):
#   jitter 4.81e-5, same_angle 3.42e-5, quarter_turn 6.15e-5, tiny_angle 4.80e-5, shift_only 5.66e-5, axis0 1.50e-5,
#   big_angle 5.19e-5, identical 2.25e-5 (19 of its 2000 pairs unstable, none in the other families)
#   -> raw 6.15e-5, rounded up to 7e-5 (DETECTOR_IOU_MEASURED, what the host test holds the restatement to; seed 2
#   gave 5.14e-5).  That is 7 x F32_IOU_NOISE, which was measured on random pairs only.
# The device's sinf / cosf / atan2f are an independent draw of the same rounding noise, hence a margin of a factor 2
# for the kernel against float64: 1.4e-4.
DETECTOR_IOU_MEASURED = 7e-5
DETECTOR_IOU_NOISE = 2 * DETECTOR_IOU_MEASURED
# The same for the overlap area, relative to the area of the smaller box of the pair: raw 3.52e-5 (jitter; seed 2
# gave 3.58e-5), rounded up to 4e-5, margin of a factor 2: 8e-5.
DETECTOR_AREA_MEASURED = 4e-5
DETECTOR_AREA_NOISE = 2 * DETECTOR_AREA_MEASURED


def _detector_sizes(rng, n):
    """(extent along x, extent along y) of vehicles, pedestrians and trucks: width 0.5 - 2.5 m, length 0.5 - 12 m"""
    kind = rng.integers(0, 3, n)
    length = np.choose(kind, [rng.uniform(3.5, 5.5, n), rng.uniform(0.5, 1.0, n), rng.uniform(6.0, 12.0, n)])
    width = np.choose(kind, [rng.uniform(1.6, 2.2, n), rng.uniform(0.5, 0.9, n), rng.uniform(2.0, 2.5, n)])
    return np.column_stack([length, width])


def _xyxyr(c, s, r):
    return np.column_stack([c - s / 2, c + s / 2, r]).astype(F32)


def detector_pairs(family, n, seed):
    """n pairs (a[i], b[i]) as a detector's near-duplicates of one object: centres within +-75 m, vehicle / pedestrian /
    truck sizes.  Box b is box a with
      jitter        centre sigma 0.15 m, size 3 %, angle sigma 0.05 rad
      same_angle    the same size and angle, the centre shifted by up to half the size along both axes
      quarter_turn  the angle + k pi / 2, k in -2 .. 2, centre sigma 0.15 m
      tiny_angle    the angle +- 10^U(-7, -3), centre sigma 0.15 m
      shift_only    the same size and angle, the centre shifted along ONE axis
      axis0         both angles 0, centre and size jitter
      big_angle     the jitter family with k 2 pi (|k| <= 20) added to either angle
      identical     nothing changed: b = a"""
    assert family in DETECTOR_FAMILIES, family
    rng = np.random.default_rng([seed, DETECTOR_FAMILIES.index(family)])
    ca = rng.uniform(-75, 75, (n, 2))
    sa = _detector_sizes(rng, n)
    ra = rng.uniform(-np.pi, np.pi, n)
    cb, sb, rb = ca.copy(), sa.copy(), ra.copy()
    near = rng.normal(0, 0.15, (n, 2))
    if family in ('jitter', 'axis0', 'big_angle'):
        cb = ca + near
        sb = sa * (1 + rng.normal(0, 0.03, (n, 2)))
        rb = ra + rng.normal(0, 0.05, n)
    if family == 'same_angle':
        cb = ca + rng.uniform(-0.5, 0.5, (n, 2)) * sa
    elif family == 'quarter_turn':
        cb = ca + near
        rb = ra + rng.integers(-2, 3, n) * (np.pi / 2)
    elif family == 'tiny_angle':
        cb = ca + near
        rb = ra + rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-7, -3, n)
    elif family == 'shift_only':
        axis = rng.integers(0, 2, n)
        cb[np.arange(n), axis] += rng.uniform(-1, 1, n) * sa[np.arange(n), axis]
    elif family == 'axis0':
        ra, rb = np.zeros(n), np.zeros(n)
    elif family == 'big_angle':
        ra = ra + rng.integers(-20, 21, n) * (2 * np.pi)
        rb = rb + rng.integers(-20, 21, n) * (2 * np.pi)
    over = np.sign(cb) * np.maximum(np.abs(cb) - 75, 0)  # a pair that left the range is moved back as a whole
    a, b = _xyxyr(ca - over, sa, ra), _xyxyr(cb - over, sb, rb)
    if family == 'identical':
        b = a.copy()
    return a, b


_OBJECT_KINDS = np.array([[4.5, 1.9], [0.8, 0.6], [1.8, 0.7], [10.0, 2.5]])  # car, pedestrian, cyclist, truck


def detector_boxes(n, seed):
    """n boxes [x1, y1, x2, y2, ry] as the raw output of a detection head, for NMS: about n / 25 objects of four size
    kinds, every box one of its object's near-duplicates (centre sigma 0.15 m, size 3 %, angle sigma 0.05 rad), 10 %
    of them flipped by pi, 10 % exact copies of an earlier box of the same object.  The objects lie within
    +-min(75, 3.5 sqrt(objects)) m, so neighbouring objects overlap now and then."""
    rng = np.random.default_rng([seed, 1000])
    n_obj = max(1, int(round(n / 25)))
    extent = min(75.0, 3.5 * np.sqrt(n_obj))
    oc = rng.uniform(-extent, extent, (n_obj, 2))
    os_ = _OBJECT_KINDS[rng.integers(0, 4, n_obj)] * rng.uniform(0.85, 1.15, (n_obj, 2))
    orot = rng.uniform(-np.pi, np.pi, n_obj)
    obj = rng.integers(0, n_obj, n)
    c = oc[obj] + rng.normal(0, 0.15, (n, 2))
    s = os_[obj] * (1 + rng.normal(0, 0.03, (n, 2)))
    r = orot[obj] + rng.normal(0, 0.05, n) + np.where(rng.random(n) < 0.1, np.pi, 0.0)
    b = _xyxyr(c, s, r)
    dup = rng.random(n) < 0.1
    pick = rng.random(n)
    seen = [[] for _ in range(n_obj)]
    for i in range(n):
        earlier = seen[obj[i]]
        if dup[i] and earlier:
            b[i] = b[earlier[int(pick[i] * len(earlier))]]
        earlier.append(i)
    return b


@functools.lru_cache(maxsize=4)
def _detector_frame(m, seed):
    """m detector_boxes in a random score order with their compared pairs, judged once: (boxes, j of every pair,
    unstable, float32 IoU, float64 IoU)"""
    b = detector_boxes(m, seed)[np.random.default_rng([seed, 2000]).permutation(m)]
    ii, jj = near_pairs(b)
    unstable, iou64 = unstable_pairs(b[ii], b[jj])
    return b, jj, unstable, bev_iou_f32(b[ii], b[jj]).astype(np.float64), iou64


def detector_nms_inputs(n, thresh, seed):
    """n detector_boxes in a random score order for rotated NMS at `thresh` -> (boxes [n, 5], share of the generated
    boxes that was dropped).  Of every compared pair that is unstable, or whose IoU (float32 or float64) is within
    2 x DETECTOR_IOU_NOISE of the threshold, the later box is dropped: the kernel and the host sweep may each differ by
    DETECTOR_IOU_NOISE from float64 on the pairs that are left.  15 % extra boxes are generated so that n stays exact."""
    m = int(n * 1.15) + 8
    b, jj, unstable, iou32, iou64 = _detector_frame(m, seed)
    bad = unstable | (np.abs(iou32 - thresh) <= 2 * DETECTOR_IOU_NOISE) | (np.abs(iou64 - thresh) <= 2 * DETECTOR_IOU_NOISE)
    drop = np.zeros(m, bool)
    drop[jj[bad]] = True
    b = b[~drop]
    assert len(b) >= n, (len(b), n)
    return b[:n].copy(), drop.sum() / m


def iou_f64_pairs(a, b):
    """the float64 clip over pairs -> (IoU, overlap area), a Python loop (about 40 us per pair)"""
    a64, b64 = np.asarray(a, np.float64).reshape(-1, 5), np.asarray(b, np.float64).reshape(-1, 5)
    area = np.array([bev_overlap_f64(x, y) for x, y in zip(a64, b64)]).reshape(-1)
    sa = (a64[:, 2] - a64[:, 0]) * (a64[:, 3] - a64[:, 1])
    sb = (b64[:, 2] - b64[:, 0]) * (b64[:, 3] - b64[:, 1])
    return area / np.maximum(sa + sb - area, 1e-8), area


def smaller_area(a, b):
    a64, b64 = np.asarray(a, np.float64).reshape(-1, 5), np.asarray(b, np.float64).reshape(-1, 5)
    return np.minimum((a64[:, 2] - a64[:, 0]) * (a64[:, 3] - a64[:, 1]), (b64[:, 2] - b64[:, 0]) * (b64[:, 3] - b64[:, 1]))


def unstable_pairs(a, b, iou64=None):
    """the pairs whose float32 restatement is more than UNSTABLE_GAP from float64 -> (bool [N], float64 IoU [N]); the
    host decides this, never a kernel's output"""
    if iou64 is None:
        iou64 = iou_f64_pairs(a, b)[0]
    return np.abs(bev_iou_f32(a, b).astype(np.float64) - iou64) > UNSTABLE_GAP, iou64


DETECTOR_PAIRS = 2000


@functools.lru_cache(maxsize=None)
def detector_family(family):
    """the committed pairs of a family with their float64 reference, computed once and shared (read only)"""
    a, b = detector_pairs(family, DETECTOR_PAIRS, DETECTOR_SEED)
    iou64, area64 = iou_f64_pairs(a, b)
    return dict(a=a, b=b, iou64=iou64, area64=area64, small=smaller_area(a, b),
                unstable=unstable_pairs(a, b, iou64)[0])


# ---------------------------------------------------------------------------------------------------------------------
# structured NMS inputs with analytic keep lists: axis-aligned boxes whose IoUs are exact in float32
# ---------------------------------------------------------------------------------------------------------------------
HALF_PAIR = np.array([[0, 0, 2, 2, 0], [0, 0, 2, 1, 0]], F32)  # IoU exactly 0.5, rotated and axis mode
BELOW_HALF = float(np.nextafter(F32(0.5), F32(0)))              # the largest float32 below 0.5


def chain_boxes(n):
    """box i = [0.25 i, 0, 0.25 i + 1, 1]: neighbours have IoU 0.75 / 1.25 = 0.6, boxes two apart 0.5 / 1.5 = 1 / 3; at
    threshold 0.5 every kept box removes exactly its successor -> (boxes, keep = the even positions)"""
    x = F32(0.25) * np.arange(n, dtype=F32)
    z = np.zeros(n, F32)
    return np.column_stack([x, z, x + F32(1), z + F32(1), z]).astype(F32), np.arange(0, n, 2)


def slot_boxes(slots):
    """unit boxes on a grid of pitch 2 (100 per row): equal slots are identical boxes (IoU 1), different slots are disjoint
    (IoU 0).  The grid keeps every coordinate below 256: from there on x - 1e-5 rounds to x in float32, and the
    reference's in-box test no longer finds a corner of an identical box."""
    slots = np.asarray(slots)
    assert slots.max(initial=0) < 100 * 127
    x, y = F32(2) * (slots % 100).astype(F32), F32(2) * (slots // 100).astype(F32)
    return np.column_stack([x, y, x + F32(1), y + F32(1), np.zeros(len(x), F32)]).astype(F32)


def periodic_boxes(n, period):
    """box i is a copy of box i mod period -> (boxes, keep = range(period)); with period 70 every 64-column word of the
    mask has its own bit pattern and each kept row's copies lie in every later column block"""
    return slot_boxes(np.arange(n) % period), np.arange(min(n, period))


def dense_boxes(n):
    """n identical boxes: every mask word is full -> (boxes, keep = [0])"""
    return slot_boxes(np.zeros(n, np.int64)), np.arange(min(n, 1))


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


def nms_inputs(n, thresh, rotated, seed):
    """sorted boxes with no compared pair's IoU within 1e-4 of the threshold(s): the later box of such a pair is
    dropped (the pairs among the boxes that stay are a subset of the pairs judged, so one pass is enough)"""
    thresholds = np.atleast_1d(np.asarray(thresh, F32))
    extent = max(8.0, np.sqrt(max(n, 1)) * 1.2)
    b = cluster_boxes(int(n * 1.1) + 4, seed, extent)
    fn = bev_iou_f32 if rotated else axis_iou_f32
    ii, jj = near_pairs(b)
    iou = fn(b[ii], b[jj]) if len(ii) else np.zeros(0, F32)
    bad = (np.abs(iou[:, None] - thresholds[None]) < 1e-4).any(1)
    drop = np.zeros(len(b), bool)
    drop[jj[bad]] = True
    return b[~drop][:n]


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
