"""Numpy float32 restatements of the reference's furthest point sampling (mmdet3d/ops/furthest_point_sample/src/
furthest_point_sample_cuda.cu:25-141, 213-331) and of the SSG flow around it (detectors/single_stage_fsd.py:83-142,
1002-1194).  Test helper: no GPU; torch only inside load_reference_ssg (the reference's own Python, where its tree is present).

Two forms of the sampling:
  fps / fps_with_dist / fps_segmented   vectorised, with the tie rule as a RANK: among equal distances the winner is the k
                                        with the smallest (bitreverse_{log2 B}(k mod B), k div B)
  fps_literal / fps_with_dist_literal   thread by thread: the strided scan of every thread and the shared-memory tree with
                                        its left-operand-wins update, for small N (pins the rank)
Distances: d = (x2-x1)*(x2-x1) + (y2-y1)*(y2-y1) + (z2-z1)*(z2-z1), left to right, each operation rounded to float32 - numpy
evaluates exactly that.
"""
import math

import numpy as np

F32 = np.float32
MULTI_BALL, EMPTY_SEGMENT, BAD_KEYPOINT = 1, 2, 4


def n_threads(n):
    """opt_n_threads of the reference (furthest_point_sample_cuda.cu:11-15), with its own floating-point log"""
    pow_2 = int(math.log(float(n)) / math.log(2.0))
    return max(min(1 << pow_2, 1024), 1)


def tie_rank(n):
    """rank[k]: the smaller, the earlier k wins among equal distances"""
    b = n_threads(n)
    lb = b.bit_length() - 1
    k = np.arange(n, dtype=np.int64)
    kmod, kdiv = k % b, k // b
    rev = np.zeros(n, np.int64)
    for bit in range(lb):
        rev |= ((kmod >> bit) & 1) << (lb - 1 - bit)
    q = (n + b - 1) // b
    return rev * q + kdiv


def lowest_index_rank(n):
    return np.arange(n, dtype=np.int64)


def sqdist(points, q):
    p = points.astype(F32, copy=False)
    dx, dy, dz = p[:, 0] - q[0], p[:, 1] - q[1], p[:, 2] - q[2]
    return (dx * dx + dy * dy) + dz * dz


def _select(temp, rank):
    cand = np.flatnonzero(temp == temp.max())
    return int(cand[np.argmin(rank[cand])])


def fps(points, m, rank=None):
    """points [n, >= 3] -> int32 [m]"""
    points = np.asarray(points, F32)
    n = len(points)
    rank = tie_rank(n) if rank is None else rank
    idx = np.zeros(m, np.int32)
    temp = np.full(n, 1e10, F32)
    old = 0
    for j in range(1, m):
        temp = np.minimum(temp, sqdist(points, points[old]))
        old = _select(temp, rank)
        idx[j] = old
    return idx


def fps_with_dist(mat, m, rank=None):
    """mat: [n, n] array, or anything with len() whose [i] is row i as a float32 array (large matrices kept elsewhere)"""
    n = len(mat)
    rank = tie_rank(n) if rank is None else rank
    idx = np.zeros(m, np.int32)
    temp = np.full(n, 1e10, F32)
    old = 0
    for j in range(1, m):
        temp = np.minimum(temp, mat[old])
        old = _select(temp, rank)
        idx[j] = old
    return idx


def fps_segmented(points, offsets, m, identity_if_short):
    """-> (idx int32 [S, m], count int32 [S]) as sst_fps_segmented_f32 documents them"""
    s = len(offsets) - 1
    idx = np.full((s, m), -1, np.int32)
    count = np.zeros(s, np.int32)
    for i in range(s):
        seg = points[offsets[i]:offsets[i + 1]]
        n = len(seg)
        if n == 0:
            continue
        if identity_if_short and n <= m:
            idx[i, :n] = np.arange(n)
            count[i] = n
        else:
            idx[i] = fps(seg, m)
            count[i] = m
    return idx, count


def _tree(dists, dists_i, b):
    """the reference's reduction: partner at +b/2 ... +1, the left operand wins unless the right is strictly larger"""
    half = b // 2
    while half >= 1:
        for tid in range(half):
            v1, v2 = dists[tid], dists[tid + half]
            i1, i2 = dists_i[tid], dists_i[tid + half]
            dists[tid] = max(v1, v2)
            dists_i[tid] = i2 if v2 > v1 else i1
        half //= 2
    return int(dists_i[0])


def _literal(n, m, dist_to):
    b = n_threads(n)
    temp = np.full(n, 1e10, F32)
    idx = np.zeros(m, np.int32)
    old = 0
    for j in range(1, m):
        d = dist_to(old)
        dists = np.zeros(b, F32)
        dists_i = np.zeros(b, np.int64)
        for tid in range(b):
            besti, best = 0, F32(-1)
            for k in range(tid, n, b):
                d2 = min(d[k], temp[k])
                temp[k] = d2
                if d2 > best:
                    besti, best = k, d2
            dists[tid], dists_i[tid] = best, besti
        old = _tree(dists, dists_i, b)
        idx[j] = old
    return idx


def fps_literal(points, m):
    points = np.asarray(points, F32)
    return _literal(len(points), m, lambda old: sqdist(points, points[old]))


def fps_with_dist_literal(mat, m):
    mat = np.asarray(mat, F32)
    return _literal(len(mat), m, lambda old: mat[old])


def lattice(n, seed, side=4):
    """integer-lattice points: many exactly equal distances"""
    return np.random.default_rng(seed).integers(0, side, (n, 3)).astype(F32)


# ----------------------------------------------------------------------------------------------------------------------
# SSG: pruning, numbering, assignment
# ----------------------------------------------------------------------------------------------------------------------
def xy_dist(a, b):
    """[len(a), len(b)] float32 sqrt(dx*dx + dy*dy) as `((a[:, None, :2] - b[None, :, :2]) ** 2).sum(2) ** 0.5`"""
    d = a[:, None, :2].astype(F32) - b[None, :, :2].astype(F32)
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])


def ssg_assign(points, offsets, key_idx, key_count, thr2, radius):
    """sst_ssg_assign_f32: -> (cluster_id int32 [n], n_clusters, status)"""
    points = np.asarray(points, F32)
    ids = np.full(len(points), -1, np.int32)
    base, status = 0, 0
    thr2, radius = F32(thr2), F32(radius)
    for s in range(len(offsets) - 1):
        seg = points[offsets[s]:offsets[s + 1]]
        if len(seg) == 0:
            continue
        keys = seg[np.asarray(key_idx[s][:key_count[s]], np.int64)]
        close = xy_dist(keys, keys) < thr2                       # [i, j]
        earlier = np.arange(len(keys))[:, None] < np.arange(len(keys))[None, :]
        valid = ~(close & earlier).any(0)
        balls = xy_dist(keys[valid], seg) < radius               # [K, n]
        hits = balls.sum(0)
        if (hits > 1).any():
            status |= MULTI_BALL
        if not (hits == 1).any():
            status |= EMPTY_SEGMENT
        which = balls.argmax(0)
        ids[offsets[s]:offsets[s + 1]] = np.where(hits == 1, which + base, -1)
        base += int(valid.sum())
    return ids, base, status


def ssg(points, batch_idx, num_fps, radius):
    """ssg() of single_stage_fsd.py:83-97 for ASCENDING batch_idx: -> (ids int32 [n], status)"""
    points = np.asarray(points, F32)
    batch_idx = np.asarray(batch_idx)
    n_samples = int(batch_idx.max()) + 1
    offsets = np.searchsorted(batch_idx, np.arange(n_samples + 1))
    key_idx, key_count = fps_segmented(points, offsets, num_fps, True)
    ids, _, status = ssg_assign(points, offsets, key_idx, key_count, F32(radius * 2 + 0.01), F32(radius))
    return ids, status


def group_means(points, cells):
    """scatter_v2(points, cells, mode='avg', return_inv=True): sorted-unique rows, float32 sums in row order / count"""
    uniq, inv = np.unique(cells, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    sums = np.zeros((len(uniq), points.shape[1]), F32)
    np.add.at(sums, inv, points.astype(F32))
    cnt = np.bincount(inv, minlength=len(uniq)).astype(F32)
    return sums / cnt[:, None], uniq, inv


def zyx_cells(points, batch_idx, vsize, pc_range):
    c = np.floor((points.astype(F32) - np.asarray(pc_range[:3], F32)) / np.asarray(vsize, F32)).astype(np.int64)
    return np.concatenate([np.asarray(batch_idx, np.int64)[:, None], c[:, ::-1]], 1)


def ssg_assigner_single_class(points, batch_idx, vsize, pc_range, num_fps, radius, per_sample):
    """SSGAssigner.forward_single_class (per_sample False: one segment) / HybridAssigner.forward_ssg (True)
    -> (rows int64 [k, 2] = (sample, id), mask bool [n])"""
    voxels, uniq, inv = group_means(points[:, :3], zyx_cells(points, batch_idx, vsize, pc_range))
    sample = uniq[:, 0] if per_sample else np.zeros(len(uniq), np.int64)
    ids, status = ssg(voxels, sample, num_fps, radius)
    assert status == 0
    per_point = ids[inv].astype(np.int64)
    mask = per_point > -1
    return np.stack([np.asarray(batch_idx, np.int64)[mask], per_point[mask]], 1), mask


def quantised_clusters(n_points, n_centres, sigma, n_samples, seed, extent=50.0, q=64.0):
    """points scattered around random centres, coordinates multiples of 1/q (sums of a few of them are exact in float32
    whatever the order), samples stored one after the other"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-extent, extent, (n_centres, 3))
    centres[:, 2] = rng.uniform(-1, 1, n_centres)
    pick = rng.integers(0, n_centres, n_points)
    pts = centres[pick] + rng.normal(0, sigma, (n_points, 3))
    pts = (np.round(pts * q) / q).astype(F32)
    batch = np.sort(rng.integers(0, n_samples, n_points)).astype(np.int64)
    return pts, batch


# ----------------------------------------------------------------------------------------------------------------------
# the reference's own functions (where its tree is present), with the sampling kernel replaced by the restatement above
# ----------------------------------------------------------------------------------------------------------------------
FAMILIES = {          # name: (radius, sigma, points, num_fps, seed)
    'car': (2.0, 0.7, 1800, 128, 11),
    'pedestrian': (0.6, 0.1, 1200, 256, 12),
    'short': (1.0, 0.3, 100, 500, 13),
}
PC_RANGE = [-64, -64, -4, 64, 64, 4]
SSG_ASSIGNER = dict(cluster_voxel_size={'Car': [0.5, 0.5, 8], 'Pedestrian': [0.25, 0.25, 8]}, point_cloud_range=PC_RANGE,
                    radius={'Car': 2.0, 'Pedestrian': 0.6}, num_fps={'Car': 128, 'Pedestrian': 256},
                    class_names=['Car', 'Pedestrian'])
HYBRID_ASSIGNER = dict(point_cloud_range=PC_RANGE, class_names=['Car', 'Pedestrian'], cfg_per_class={
    'Car': dict(assigner_type='ssg', cluster_voxel_size=[0.5, 0.5, 8], radius=2.0, num_fps=128),
    'Pedestrian': dict(assigner_type='ccl', cluster_voxel_size=[0.25, 0.25, 8], min_points=2, connected_dist=0.6)})
CLASS_FAMILY = {'Car': 'car', 'Pedestrian': 'pedestrian'}


def family(name):
    radius, sigma, n, num_fps, seed = FAMILIES[name]
    pts, batch = quantised_clusters(n, 60, sigma, 3, seed)
    return pts, batch, num_fps, radius


def load_reference_ssg():
    """fps / ssg_single_sample / ssg / SSGAssigner / HybridAssigner executed from the reference's own source text
    (oracle.ref_loader), on CPU tensors; `furthest_point_sample` is fps() above."""
    import types

    import torch
    from oracle import ref_loader
    from oracle.ref_fsd import _FSD, _multi_apply
    from scipy.sparse.csgraph import connected_components

    def furthest_point_sample(points_xyz, num_points):
        return torch.from_numpy(np.stack([fps(p.numpy(), num_points) for p in points_xyz]))

    ref = ref_loader.load_reference()
    glb = {'scatter_v2': ref.sst_ops.scatter_v2, 'multi_apply': _multi_apply, 'connected_components': connected_components,
           'furthest_point_sample': furthest_point_sample}
    for fn in ('fps', 'ssg_single_sample', 'ssg', 'filter_almost_empty', 'find_connected_componets',
               'find_connected_componets_single_batch', 'modify_cluster_by_class'):
        glb[fn] = ref_loader.load_reference_function(_FSD, fn, glb)
    glb['SSGAssigner'] = ref_loader.load_reference_class(_FSD, 'SSGAssigner', glb)
    # HybridAssigner.forward_ccl hands find_connected_componets the int64 sample column of its int64 coordinates, and that
    # function's `components_inds[batch_mask] = c_inds` (int32 labels into a zeros_like of the column) is refused by torch
    # ("Index put requires the source and destination dtypes match").  The column is cast to int32 on the way in - the
    # dtype ClusterAssigner passes - so that the branch can be executed at all; labels and rows are unchanged by it.
    components = glb['find_connected_componets']
    hybrid_glb = dict(glb, find_connected_componets=lambda points, batch_idx, dist: components(points, batch_idx.int(), dist))
    glb['HybridAssigner'] = ref_loader.load_reference_class(_FSD, 'HybridAssigner', hybrid_glb)
    return types.SimpleNamespace(**{k: glb[k] for k in ('fps', 'ssg_single_sample', 'ssg', 'SSGAssigner', 'HybridAssigner')})


def ccl_assigner_single_class(points, batch_idx, vsize, pc_range, min_points, dist):
    """HybridAssigner.forward_ccl (single_stage_fsd.py:1164-1194): -> (rows int64 [k, 2], mask bool [n])"""
    from oracle import cluster_oracle
    cells = zyx_cells(points, batch_idx, vsize, pc_range)
    _, inv, cnt = np.unique(cells, axis=0, return_inverse=True, return_counts=True)
    mask = cnt[inv.reshape(-1)] >= min_points
    if not mask.any():
        mask = ~mask
    centres, uniq, inv2 = group_means(points[mask, :3], cells[mask])
    labels = cluster_oracle.find_connected_components(centres, uniq[:, 0], dist).astype(np.int64)
    return np.stack([np.asarray(batch_idx, np.int64)[mask], labels[inv2]], 1), mask
