"""Float32 numpy restatement of the training augmentation (sst_amd/augment.py, csrc/augment.hip), operation by operation, written
from the reference's sources: mmdet3d/datasets/pipelines/transforms_3d.py (ObjectSample :262-334, RandomFlip3D :95-172,
GlobalRotScaleTrans :564-676, ObjectRangeFilter, PointsRangeFilter), mmdet3d/core/bbox/structures/lidar_box3d.py:143-248,
base_box3d.py:222-245, mmdet3d/core/points/base_points.py:139-229 and mmdet3d/core/bbox/box_np_ops.py:205-234, :403-445, :693-752.
tests/test_augment_host.py pins it to the reference's classes; tests/test_gpu_augment.py pins the kernels to it bit by bit."""
import numpy as np

F = np.float32
PI32 = F(np.pi)
GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def box_planes(boxes):
    """float32 [S, >= 7] -> float32 [S, 6, 4]: (a, b, c, d) of the six faces, normals inwards; center_to_corner_box3d with
    origin (0.5, 0.5, 0) and axis 2, corner_to_surfaces_3d, surface_equ_3d"""
    b = np.asarray(boxes, F).reshape(-1, np.shape(boxes)[-1])[:, :7]
    if b.shape[0] == 0:
        return np.zeros((0, 6, 4), F)
    norm = np.stack(np.unravel_index(np.arange(8), [2] * 3), axis=1).astype(F)[[0, 1, 3, 2, 4, 5, 7, 6]]
    norm = norm - np.array((0.5, 0.5, 0), dtype=F)
    corners = b[:, 3:6].reshape([-1, 1, 3]) * norm.reshape([1, 8, 3])
    rot_sin, rot_cos = np.sin(b[:, 6]), np.cos(b[:, 6])
    ones, zeros = np.ones_like(rot_cos), np.zeros_like(rot_cos)
    rot_mat_T = np.stack([[rot_cos, -rot_sin, zeros], [rot_sin, rot_cos, zeros], [zeros, zeros, ones]])
    corners = np.einsum('aij,jka->aik', corners, rot_mat_T)
    corners += b[:, :3].reshape([-1, 1, 3])
    quads = ((0, 1, 2, 3), (7, 6, 5, 4), (0, 3, 7, 4), (1, 5, 6, 2), (0, 4, 5, 1), (3, 2, 6, 7))
    surfaces = np.array([[corners[:, k] for k in q] for q in quads]).transpose([2, 0, 1, 3])
    vec = surfaces[:, :, :2, :] - surfaces[:, :, 1:3, :]
    normal = np.cross(vec[:, :, 0, :], vec[:, :, 1, :])
    d = np.einsum('aij, aij->ai', normal, surfaces[:, :, 0, :])
    return np.concatenate([normal, -d[..., None]], -1).astype(F)


def points_in_planes(xyz, planes):
    """bool [N, S]: sgn = ((x a + y b) + z c) + d < 0 for all six faces; sgn >= 0 is outside (box_np_ops.py:745-751)"""
    xyz = np.asarray(xyz, F)
    x, y, z = (xyz[:, k, None, None] for k in range(3))
    p = np.asarray(planes, F)[None]
    with np.errstate(invalid='ignore', over='ignore'):
        sgn = ((x * p[..., 0] + y * p[..., 1]) + z * p[..., 2]) + p[..., 3]
        return (sgn < 0).all(-1)


def shuffle_keys(seed, sample, n):
    """uint32 [n]: the high word of splitmix64's finaliser over seed + GOLDEN * (((sample << 32) | row) + 1), modulo 2^64"""
    with np.errstate(over='ignore'):
        x = np.uint64(seed) + GOLDEN * (((np.uint64(sample) << np.uint64(32)) | np.arange(n, dtype=np.uint64)) + np.uint64(1))
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (x >> np.uint64(32)).astype(np.uint32)


def flip_points(xyz, flip_h, flip_v):
    xyz = np.asarray(xyz, F).copy()
    if flip_h:
        xyz[:, 1] = -xyz[:, 1]
    if flip_v:
        xyz[:, 0] = -xyz[:, 0]
    return xyz


def rotate_xy(x, y, c, s):
    """x' = x c + y s, y' = x (-s) + y c: ``[x, y] @ [[c, -s], [s, c]]`` written out, each operation rounded on its own"""
    c, s = F(c), F(s)
    with np.errstate(invalid='ignore', over='ignore'):
        return (x * c + y * s).astype(F), (x * (-s) + y * c).astype(F)


def rotate_points(xyz, c, s):
    xyz = np.asarray(xyz, F).copy()
    xyz[:, 0], xyz[:, 1] = rotate_xy(xyz[:, 0].copy(), xyz[:, 1].copy(), c, s)
    return xyz


def scale_points(xyz, scale):
    with np.errstate(invalid='ignore', over='ignore'):
        return (np.asarray(xyz, F) * F(scale)).astype(F)


def translate_points(xyz, trans):
    with np.errstate(invalid='ignore', over='ignore'):
        return (np.asarray(xyz, F) + np.asarray(trans, F)[None]).astype(F)


def transform_points(xyz, rec):
    """flips, rotation, scale, translation of float32 [N, 3]; ``rec``: one record (flip_h, flip_v, rotate, cos, sin, scale, trans)"""
    xyz = flip_points(np.asarray(xyz, F)[:, :3], rec['flip_h'], rec['flip_v'])
    if rec['rotate']:
        xyz = rotate_points(xyz, rec['cos'], rec['sin'])
    return translate_points(scale_points(xyz, rec['scale']), rec['trans'])


def in_range_3d(xyz, r):
    r = np.asarray(r, F)
    with np.errstate(invalid='ignore'):
        return ((xyz[:, 0] > r[0]) & (xyz[:, 1] > r[1]) & (xyz[:, 2] > r[2]) & (xyz[:, 0] < r[3]) & (xyz[:, 1] < r[4])
                & (xyz[:, 2] < r[5]))


def augment_points(rows, n_pasted, planes, rec, sample, norm=None):
    """one sample: rows float32 [N, C] with the n_pasted pasted rows first -> (output rows [M, C], the input row of every
    output row int64 [M])"""
    rows = np.asarray(rows, F)
    n = rows.shape[0]
    inside = np.zeros(n, bool)
    if len(planes):
        inside[n_pasted:] = points_in_planes(rows[n_pasted:, :3], planes).any(-1)
    xyz = transform_points(rows[:, :3], rec)
    keep = ~inside & in_range_3d(xyz, rec['range'])
    idx = np.nonzero(keep)[0]
    if rec['shuffle']:
        idx = idx[np.argsort(shuffle_keys(rec['seed'], sample, n)[idx], kind='stable')]
    out = np.concatenate([xyz, rows[:, 3:]], 1)[idx]
    if norm is not None:
        for k, m, s in zip(*norm):
            if k < out.shape[1]:
                out[:, k] = (out[:, k] - F(m)) / F(s)
    return out.astype(F), idx


def limit_period(val, offset, period):
    val = np.asarray(val, F)
    return (val - np.floor(val / F(period) + F(offset)) * F(period)).astype(F)


def flip_boxes(boxes, flip_h, flip_v):
    b = np.asarray(boxes, F).copy()
    if flip_h:
        b[:, 1::7] = -b[:, 1::7]
        b[:, 6] = -b[:, 6] + PI32
    if flip_v:
        b[:, 0::7] = -b[:, 0::7]
        b[:, 6] = -b[:, 6]
    return b


def rotate_boxes(boxes, c, s, angle):
    b = np.asarray(boxes, F).copy()
    b[:, 0], b[:, 1] = rotate_xy(b[:, 0].copy(), b[:, 1].copy(), c, s)
    with np.errstate(invalid='ignore'):
        b[:, 6] = b[:, 6] + F(angle)
    if b.shape[1] == 9:
        b[:, 7], b[:, 8] = rotate_xy(b[:, 7].copy(), b[:, 8].copy(), c, s)
    return b


def scale_boxes(boxes, scale):
    b = np.asarray(boxes, F).copy()
    with np.errstate(invalid='ignore', over='ignore'):
        b[:, :6] *= F(scale)
        if b.shape[1] > 7:
            b[:, 7:9] *= F(scale)
    return b


def translate_boxes(boxes, trans):
    b = np.asarray(boxes, F).copy()
    with np.errstate(invalid='ignore', over='ignore'):
        b[:, :3] += np.asarray(trans, F)[None]
    return b


def in_range_bev(boxes, r):
    r = np.asarray(r, F)
    with np.errstate(invalid='ignore'):
        return (boxes[:, 0] > r[0]) & (boxes[:, 1] > r[1]) & (boxes[:, 0] < r[3]) & (boxes[:, 1] < r[4])


def limit_yaw(boxes):
    b = np.asarray(boxes, F).copy()
    with np.errstate(invalid='ignore'):
        b[:, 6] = limit_period(b[:, 6], 0.5, 2 * np.pi)
    return b


def transform_boxes(boxes, rec, rotate=None, filter=True):
    """one sample's boxes float32 [G, 7 | 9] -> (kept boxes in their order, keep mask); without ``filter`` (seed boxes)
    nothing is dropped and the yaw is not limited"""
    b = flip_boxes(boxes, rec['flip_h'], rec['flip_v'])
    if bool(rec['rotate']) if rotate is None else rotate:
        b = rotate_boxes(b, rec['cos'], rec['sin'], rec['angle'])
    b = translate_boxes(scale_boxes(b, rec['scale']), rec['trans'])
    keep = np.ones(b.shape[0], bool)
    if filter:
        keep = in_range_bev(b, rec['range'])
        b = limit_yaw(b[keep])
    return b.astype(F), keep


def load_golden(golden_dir):
    """the three files tools/make_augment_golden.py writes, as one dictionary"""
    import os
    out = {}
    for name in ('augment_golden.npz', 'augment_golden_s0.npz', 'augment_golden_s1.npz'):
        with np.load(os.path.join(golden_dir, name)) as z:
            out.update({k: z[k] for k in z.files})
    return out


def golden_run(g, fh, fv, si):
    """one end-to-end case of the golden: the inputs as the pipeline sees them and the reference's arrays after every stage"""
    pre = f'e2e_h{fh}v{fv}_smp{si}_'
    r = {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}
    r['in_points'] = g[f'scene{si}_points'][r['keep_points']]
    r['in_gt'], r['in_gt_labels'] = g[f'scene{si}_gt'][r['keep_gt']], g[f'scene{si}_gt_labels'][r['keep_gt']]
    for k in ('pasted', 'pasted_labels', 'pasted_points'):
        r[k] = g[f'scene{si}_{k}']
    r['s0_points'] = np.concatenate([r['pasted_points'], r['in_points'][r['kept_own']]])
    r['s0_boxes'] = np.concatenate([r['in_gt'], r['pasted']])
    n_p = r['pasted_points'].shape[0]
    r['s0_rows'] = np.concatenate([np.arange(n_p), n_p + np.nonzero(r['kept_own'])[0]])   # the input row of every s0 row
    r['rec'] = dict(flip_h=fh, flip_v=fv, rotate=1, shuffle=0, cos=r['rot_mat_T'][0, 0], sin=r['rot_mat_T'][1, 0],
                    scale=F(r['scale']), angle=F(r['angle']), trans=r['trans'].astype(F),
                    range=np.array([-74.88, -74.88, -2, 74.88, 74.88, 4], F), seed=0)
    return r
