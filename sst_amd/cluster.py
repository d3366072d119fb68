"""FSD's cluster assignment on the GPU.

Mirrors the module-level helpers and ``ClusterAssigner`` of mmdet3d/models/detectors/single_stage_fsd.py
(:30-68 filter_almost_empty / find_connected_componets*, :144-151 modify_cluster_by_class, :922-999
ClusterAssigner): same names, arguments and return values, so ``single_stage_fsd.py`` can import them from here.

Reference cost being removed: per class and per sample a dense N x N distance matrix, a device->host copy, scipy's
connected_components on the CPU and a host->device copy (the documented source of FSD's training-time instability,
docs/overall_instructions.md:51).  Here one lock-free union-find launch over all samples (csrc/cluster.hip); labels
are bit-identical (components numbered by their smallest member, scipy's order of first appearance).

``fps`` / ``ssg_single_sample`` / ``ssg`` (:24-28, :83-142), ``SSGAssigner`` (:1002-1101) and ``HybridAssigner``
(:1104-1194) are the reference's other two assigner branches.  Reference cost being removed: a strictly sequential
sampling kernel with ten barriers per sample, three dense matrices ([K, K], [K, N] distances and the [K, N] mask),
nonzero, a sort and one read-back per assert, and in the hybrid assigner a Python loop over the samples.  Here one
sampling launch and one assignment launch sequence for all samples of a class (csrc/fps.hip), and one read-back.
"""
import ctypes

import torch

from . import _lib
from . import fps as _fps
from . import kernels as K
from .sst_ops import scatter_v2


def connected_components_xy(points, batch_idx, dist, return_count=False):
    """labels [N] int32 of the components of {same sample, xy distance < dist}; samples must be stored one after
    the other (ascending ``batch_idx``) for the numbering to equal the reference's running-base numbering."""
    if not points.is_cuda:
        raise RuntimeError('sst_amd.connected_components_xy: CUDA tensors required (no CPU fallback)')
    n = points.size(0)
    pts = points.float()
    if pts.stride(1) != 1:
        pts = pts.contiguous()
    b = batch_idx.to(torch.int32).contiguous()
    labels = torch.empty(n, dtype=torch.int32, device=points.device)
    count = torch.zeros(1, dtype=torch.int32, device=points.device)
    lib = _lib.load()
    ws = _lib.workspace(lib.sst_connected_components_workspace_bytes(n), points.device)
    rc = lib.sst_connected_components_xy_f32(_lib.ptr(pts), pts.stride(0) if n > 0 else 2, _lib.ptr(b), n, float(dist),
                                             _lib.ptr(labels), _lib.ptr(count), _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, 'sst_connected_components_xy_f32')
    return (labels, count) if return_count else labels


def filter_almost_empty(coors, min_points):
    """mask of the rows whose coordinate occurs at least ``min_points`` times (single_stage_fsd.py:30-34)."""
    if coors.size(0) == 0:
        return torch.zeros(0, dtype=torch.bool, device=coors.device)
    plan = K.unique_rows(coors.contiguous())
    cnt_per_point = plan.counts()[plan.inverse.long()]
    return cnt_per_point >= min_points


def find_connected_componets(points, batch_idx, dist):
    """single_stage_fsd.py:45-68 (training path): int labels, numbered per sample with a running base."""
    assert len(points) > 0
    b = batch_idx.int()
    sorted_already = True
    if b.numel() > 1 and points.is_cuda:
        # the centres come out of a sorted-unique, i.e. sample after sample; anything else is brought into that
        # order first (stable), labelled, and put back
        sorted_already = bool((b[1:] >= b[:-1]).all().item()) if b.numel() < (1 << 16) else None
        if sorted_already is None:
            sorted_already = bool((b[1:] >= b[:-1]).all().item())
    if sorted_already:
        labels = connected_components_xy(points, b, dist)
    else:
        order = torch.sort(b, stable=True)[1]
        lab_sorted = connected_components_xy(points[order], b[order], dist)
        labels = torch.empty_like(lab_sorted)
        labels[order] = lab_sorted
    return labels.to(batch_idx.dtype) if batch_idx.dtype != torch.int32 else labels


def find_connected_componets_single_batch(points, batch_idx, dist):
    """single_stage_fsd.py:70-84 (test path): ONE graph over all points, the sample index is ignored."""
    zeros = torch.zeros(points.size(0), dtype=torch.int32, device=points.device)
    return connected_components_xy(points, zeros, dist)


def modify_cluster_by_class(cluster_inds_list):
    """prepend the class index as column 0 (single_stage_fsd.py:144-151)."""
    new_list = []
    for i, inds in enumerate(cluster_inds_list):
        cls_pad = inds.new_ones((len(inds),)) * i
        new_list.append(torch.cat([cls_pad[:, None], inds], 1))
    return new_list


class ClusterAssigner(torch.nn.Module):
    """Cluster centres per class and the assignment of every foreground point to one of them
    (single_stage_fsd.py:922-999; same constructor and forward)."""

    def __init__(self, cluster_voxel_size, min_points, point_cloud_range, connected_dist,
                 class_names=['Car', 'Cyclist', 'Pedestrian'], gpu_clustering=(False, False)):
        super().__init__()
        self.cluster_voxel_size = cluster_voxel_size
        self.min_points = min_points
        self.connected_dist = connected_dist
        self.point_cloud_range = point_cloud_range
        self.class_names = class_names
        self.gpu_clustering = gpu_clustering
        self.num_classes = len(class_names)

    def _per_class(self, table, class_name):
        if isinstance(table, dict):
            return table[class_name]
        if isinstance(table, list):
            return table[self.class_names.index(class_name)]
        return table

    class_batched = False      # opt-in (enable_class_batched): all classes in one pass, one host read (cluster_assign_classes)

    @torch.no_grad()
    def forward(self, points_list, batch_idx_list, gt_bboxes_3d=None, gt_labels_3d=None, origin_points=None):
        assert self.num_classes == len(self.class_names)
        if self.class_batched:
            # as the zip below: the lists and the names are cut to the shortest of the three
            names = self.class_names[:min(len(points_list), len(batch_idx_list), len(self.class_names))]
            g = len(names)
            if g == 0:                                   # no list or no name: the loop below returns two empty lists
                return [], []
            inds3, masks, _ = _assign_classes(
                list(points_list[:g]), list(batch_idx_list[:g]), [self._per_class(self.cluster_voxel_size, c) for c in names],
                [self._per_class(self.connected_dist, c) for c in names], self.min_points, self.point_cloud_range[:3],
                per_sample=self.training)
            return inds3, masks
        outs = [self.forward_single_class(p, b, c, origin_points)
                for p, b, c in zip(points_list, batch_idx_list, self.class_names)]
        cluster_inds_list = modify_cluster_by_class([o[0] for o in outs])
        return cluster_inds_list, [o[1] for o in outs]

    def forward_single_class(self, points, batch_idx, class_name, origin_points):
        """One class: cluster-voxel grouping of the voted centres -> centroids of the voxels with at least ``min_points``
        votes -> connected components of the centroids -> every surviving point inherits its voxel's component
        (single_stage_fsd.py:953-999).  ONE sorted-unique grouping serves the occupancy filter, the centroid reduction and
        the point -> centroid map (the reference groups the same keys three times: filter_almost_empty, scatter_v2 and its
        inverse), and the two data-dependent lengths (surviving points, surviving voxels) are read back together."""
        dev = points.device
        batch_idx = batch_idx.int()
        cell = K.const_tensor(self._per_class(self.cluster_voxel_size, class_name), dev, points.dtype)
        origin = K.const_tensor(self.point_cloud_range[:3], dev, points.dtype)
        cells = torch.cat([batch_idx[:, None], torch.div(points - origin, cell, rounding_mode='floor').int()], dim=1)
        # the reference's test path clusters all samples as one graph (both of its variants, :36-43 / :70-84)
        return _ccl_single_class(points, batch_idx, cells, self.min_points, self._per_class(self.connected_dist, class_name),
                                 per_sample=self.training)


def _ccl_single_class(points, batch_idx, cells, min_points, dist, per_sample):
    """the grouping -> filter -> centroids -> components -> points chain of ClusterAssigner.forward_single_class and
    HybridAssigner.forward_ccl; ``cells`` [N, 4] = (sample, cluster-voxel coordinates) in the caller's column order"""
    dev = points.device
    n = points.size(0)
    if n == 0:
        empty = torch.zeros((0, 2), dtype=batch_idx.dtype, device=dev)
        return empty, torch.zeros(0, dtype=torch.bool, device=dev)
    groups = K.unique_rows(cells.contiguous())
    occupancy = groups.counts()                                         # votes per cluster voxel, sorted-voxel order
    crowded = occupancy >= min_points
    point_group = groups.inverse.long()
    valid_mask = crowded[point_group]
    sizes = torch.stack([valid_mask.sum(), crowded.sum()]).tolist()     # the one read-back of this class
    if sizes[0] == 0:
        # nothing survives the filter: the reference then keeps EVERY point (valid_mask = ~valid_mask, :968-970)
        valid_mask = torch.ones_like(valid_mask)
        crowded = torch.ones_like(crowded)
        sizes = [n, groups.m]
    keep_points = _nonzero_known(valid_mask, sizes[0])
    keep_groups = _nonzero_known(crowded, sizes[1])
    # centroids of the surviving voxels: the mean over ALL votes of a voxel (a voxel survives or falls as a whole)
    centroids = K.segment_reduce(points.float().contiguous(), groups, 'mean').index_select(0, keep_groups)
    centroid_sample = K.unpack_unique_rows(groups, torch.int32).index_select(0, keep_groups)[:, 0]
    if per_sample:
        component = connected_components_xy(centroids, centroid_sample, dist)   # sorted-unique order = sample after sample
    else:
        component = find_connected_componets_single_batch(centroids, centroid_sample, dist)
    assert component.numel() == sizes[1]
    rank_of_group = torch.cumsum(crowded.int(), 0) - 1                   # surviving voxel -> row of `centroids`
    point_component = component[rank_of_group[point_group[keep_points]].long()]
    valid_mask._sst_keep = keep_points     # the indices of the set entries ride along: callers need not search again
    return torch.stack([batch_idx[keep_points], point_component.to(batch_idx.dtype)], 1), valid_mask


def _nonzero_known(mask, count):
    """indices of the set entries of a 1-D mask whose number is already on the host: no further read-back"""
    if hasattr(torch, 'nonzero_static'):
        return torch.nonzero_static(mask, size=int(count)).squeeze(1)
    return torch.nonzero(mask).squeeze(1)


# ----------------------------------------------------------------------------------------------------------------------
# all classes in one pass (csrc/cluster_classes.hip)
# ----------------------------------------------------------------------------------------------------------------------
MAX_BATCHED_CLASSES = 32
MAX_BATCHED_SAMPLES = 256


def enable_class_batched(module, on=True):
    """set ``class_batched`` on every ClusterAssigner below ``module`` (the module itself included): their ``forward`` then
    clusters all classes in one pass with one host read (``cluster_assign_classes``).  -> the number of assigners found"""
    found = 0
    for m in module.modules():
        if isinstance(m, ClusterAssigner):
            m.class_batched = bool(on)
            found += 1
    return found


def _class_tables(n_classes, cell_sizes, dists):
    cells, ds = [], []
    if len(cell_sizes) != n_classes or len(dists) != n_classes:
        raise ValueError(f'sst_amd.cluster_assign_classes: {n_classes} classes, but {len(cell_sizes)} cell sizes and '
                         f'{len(dists)} distances')
    for c in range(n_classes):
        cell = [float(v) for v in cell_sizes[c]]
        if len(cell) != 3 or not all(v > 0 for v in cell):
            raise ValueError(f'sst_amd.cluster_assign_classes: cell size of class {c} must be three positive numbers, got {cell}')
        d = float(dists[c])
        if d != d:
            raise ValueError(f'sst_amd.cluster_assign_classes: connected distance of class {c} is not a number')
        cells.append(cell)
        ds.append(d)
    return cells, ds


def _assign_classes(points_list, batch_idx_list, cell_sizes, dists, min_points, origin, per_sample, count_tiles=False):
    """-> ([n_c', 3] int32 (class, sample, component) per class, valid masks with ``_sst_keep`` per class, stats)"""
    G = len(points_list)
    if G < 1 or len(batch_idx_list) != G:
        raise ValueError(f'sst_amd.cluster_assign_classes: {G} point lists and {len(batch_idx_list)} sample-index lists')
    if G > MAX_BATCHED_CLASSES:
        raise NotImplementedError(f'sst_amd.cluster_assign_classes: {G} classes; the class-batched pass covers at most '
                                  f'{MAX_BATCHED_CLASSES}')
    cells, ds = _class_tables(G, cell_sizes, dists)
    if len(origin) != 3:
        raise ValueError('sst_amd.cluster_assign_classes: origin must be (x, y, z)')
    for c, (p, b) in enumerate(zip(points_list, batch_idx_list)):
        if not (p.is_cuda and b.is_cuda):
            raise RuntimeError('sst_amd.cluster_assign_classes: CUDA tensors required (no CPU fallback)')
        if p.dtype != torch.float32 or p.dim() != 2 or p.size(1) != 3:
            raise RuntimeError(f'sst_amd.cluster_assign_classes: points of class {c} must be float32 [n, 3]')
        if b.dim() != 1 or b.size(0) != p.size(0) or b.dtype not in (torch.int32, torch.int64):
            raise RuntimeError(f'sst_amd.cluster_assign_classes: sample indices of class {c} must be int32 / int64 [n]')
    dev = points_list[0].device
    offs = [0]
    for p in points_list:
        offs.append(offs[-1] + p.size(0))
    n = offs[-1]
    if n >= 1 << 31:
        raise NotImplementedError('sst_amd.cluster_assign_classes: 2^31 votes or more')
    stats = dict(host_reads=0, n=n, centroids=0, tiles_run=0, tiles_skipped=0)
    if n == 0:
        empty = [(torch.zeros((0, 3), dtype=torch.int32, device=dev), _empty_mask(dev)) for _ in range(G)]
        return [e[0] for e in empty], [e[1] for e in empty], stats
    lib = _lib.load()
    P = _lib.ClusterClassesParams()
    P.n_classes, P.per_sample, P.min_points, P.count_tiles = G, int(bool(per_sample)), int(min_points), int(bool(count_tiles))
    for c in range(G + 1):
        P.class_off[c] = offs[c]
    for c in range(G):
        for d in range(3):
            P.cell[c][d] = cells[c][d]
        P.dist[c] = ds[c]
    for d in range(3):
        P.origin[d] = float(origin[d])
    pts = torch.cat(points_list, 0) if G > 1 else points_list[0].contiguous()
    batch = torch.cat([b.int() for b in batch_idx_list], 0) if G > 1 else batch_idx_list[0].int().contiguous()
    rows = torch.empty((n, 5), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    st = _lib.stream_ptr()
    _lib.check(lib.sst_cluster_classes_keys_f32(_lib.ptr(pts), pts.stride(0), _lib.ptr(batch), n, ctypes.byref(P), _lib.ptr(rows),
                                                _lib.ptr(status), st), 'sst_cluster_classes_keys_f32')
    mins, extents = (ctypes.c_int64 * 5)(), (ctypes.c_int64 * 5)()
    _lib.check(lib.sst_cluster_classes_key_layout(G, mins, extents), 'sst_cluster_classes_key_layout')
    # ONE sorted-unique over a key layout that no read-back sizes; its group count stays on the device
    groups = K.unique_rows(rows, mins=list(mins), extents=list(extents), defer_count=True)
    # ONE segmented mean: group g -> row g, rows behind the device-side group count are not written (and not read below)
    every_group = torch.arange(n, dtype=torch.int32, device=dev)
    centroids = K.segment_reduce(pts, groups, 'mean', group_index=every_group, inverse=groups.inverse, m_limit=groups.num)
    inds = torch.empty((n, 3), dtype=torch.int32, device=dev)
    keep = torch.empty(n, dtype=torch.int64, device=dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    sizes = torch.empty(2 * G + 4, dtype=torch.int32, device=dev)
    ws = _lib.workspace(lib.sst_cluster_classes_workspace_bytes(n), dev)
    _lib.check(lib.sst_cluster_classes_f32(_lib.ptr(centroids), _lib.ptr(rows), _lib.ptr(groups.perm), _lib.ptr(groups.offsets),
                                           _lib.ptr(groups.inverse), _lib.ptr(groups.num), n, ctypes.byref(P), _lib.ptr(status),
                                           _lib.ptr(inds), _lib.ptr(keep), _lib.ptr(mask), _lib.ptr(sizes), _lib.ptr(ws), st),
               'sst_cluster_classes_f32')
    sizes = sizes.tolist()                                              # the one read-back of all classes
    stats.update(host_reads=1, centroids=sizes[2 * G + 1], tiles_run=sizes[2 * G + 2], tiles_skipped=sizes[2 * G + 3])
    if sizes[2 * G] & 2:
        raise RuntimeError(f'sst_amd.cluster_assign_classes: a sample index outside [0, {MAX_BATCHED_SAMPLES})')
    if sizes[2 * G] & 1:
        raise RuntimeError('sst_amd.cluster_assign_classes: a vote lies further from the origin than the fixed key layout '
                           'covers (65536 cells in x and y, 16384 in z)')
    mask = mask.view(torch.bool)
    inds_list, mask_list, pos = [], [], 0
    for c in range(G):
        k = sizes[c]
        m = mask[offs[c]:offs[c + 1]]
        m._sst_keep = keep[pos:pos + k]      # the indices of the set entries ride along, as on the per-class path
        inds_list.append(inds[pos:pos + k])
        mask_list.append(m)
        pos += k
    return inds_list, mask_list, stats


def _empty_mask(dev):
    m = torch.zeros(0, dtype=torch.bool, device=dev)
    m._sst_keep = torch.zeros(0, dtype=torch.int64, device=dev)
    return m


@torch.no_grad()
def cluster_assign_classes(points_list, batch_idx_list, cell_sizes, dists, min_points, origin, per_sample):
    """What the per-class loop of ``ClusterAssigner.forward`` returns before ``modify_cluster_by_class`` - per class
    ((sample, component) int32 [n', 2], valid mask bool [n] with its index list as ``_sst_keep``) - for up to 32 classes in
    ONE pass: one key launch over the concatenated votes ((class, sample, cell) with the class's cell size, the cell being
    ``torch.div(p - origin, cell, rounding_mode='floor').int()`` bit for bit), one sorted-unique, one segmented mean, the
    occupancy filter with the reference's keep-everything rule decided per class on the device, one connected-components pass
    over the centroids of all classes (partition (class, sample) with ``per_sample``, else (class): the reference's test path
    clusters all samples as one graph; ``dists[c]`` per class), and ONE host read (the 2 G sizes).

    ``cell_sizes``: per class (x, y, z); ``dists``: per class.  The centroid of a cluster voxel is the segmented mean of the
    library over the one grouping; where three or more votes share a voxel its float sum may associate differently from the
    per-class grouping's (the reduction kernels pick their walk by the shape of the whole call), which can move a centroid by
    an ulp.  Sums that are exact in fp32, and voxels of one or two votes, give the per-class path's bits."""
    inds3, masks, _ = _assign_classes(points_list, batch_idx_list, cell_sizes, dists, min_points, origin, per_sample)
    return [(i[:, 1:], m) for i, m in zip(inds3, masks)]


# ----------------------------------------------------------------------------------------------------------------------
# furthest point sampling + ball assignment: SSGAssigner / HybridAssigner
# ----------------------------------------------------------------------------------------------------------------------
def fps(points, N):
    """the N furthest-point samples of points [n, 3], as rows (single_stage_fsd.py:24-28)"""
    idx = _fps.furthest_point_sample(points.unsqueeze(0), N)
    idx = idx.squeeze(0).long()
    return points[idx]


def _ssg_segments(points, seg_offsets, num_fps, radius):
    """sampling + pruning + numbering + assignment inside every segment of ``points``: two native calls, nothing read back.
    -> (ids int32 [n], n_clusters int32 [1], status int32 [1])"""
    pts = points.float()
    if pts.dim() != 2 or (pts.size(0) > 0 and pts.stride(1) != 1):
        pts = pts.contiguous()
    key_idx, key_count = _fps.fps_segmented(pts, seg_offsets, num_fps, identity_if_short=True)
    return _fps.ssg_assign(pts, seg_offsets, key_idx, key_count, radius * 2 + 0.01, radius)


def _one_segment(n, device):
    return torch.tensor([0, n], dtype=torch.int32, device=device)


def _segments_of_sorted(batch_sorted, n_samples):
    """offsets [n_samples + 1] of the runs of an ascending int32 sample-index vector"""
    marks = torch.arange(n_samples + 1, dtype=torch.int32, device=batch_sorted.device)
    return torch.searchsorted(batch_sorted.contiguous(), marks).int()


def ssg_single_sample(points, num_fps, radius):
    """single_stage_fsd.py:99-142: cluster id per point (-1: in no ball), int64"""
    if not points.is_cuda:
        raise RuntimeError('sst_amd.ssg_single_sample: CUDA tensors required (no CPU fallback)')
    ids, _, status = _ssg_segments(points, _one_segment(points.size(0), points.device), num_fps, radius)
    if points.size(0):
        _fps.raise_on_status(status.item())
    return ids.long()


def ssg(points, batch_idx, num_fps, radius):
    """single_stage_fsd.py:83-97 as ONE segmented call: the samples are the segments, the ids run on from sample to
    sample.  Two read-backs: the number of samples (with the order check) and the status word."""
    if not points.is_cuda:
        raise RuntimeError('sst_amd.ssg: CUDA tensors required (no CPU fallback)')
    n = points.size(0)
    if n == 0:
        return torch.zeros_like(batch_idx)
    b = batch_idx.int()
    ascending = (b[1:] >= b[:-1]).all() if n > 1 else torch.ones((), dtype=torch.bool, device=b.device)
    n_samples, sorted_already = torch.stack([b.max() + 1, ascending.to(b.dtype)]).tolist()
    if sorted_already:
        ids, _, status = _ssg_segments(points, _segments_of_sorted(b, n_samples), num_fps, radius)
    else:
        # as find_connected_componets: bring the samples one after the other (stable), label, put back
        order = torch.sort(b, stable=True)[1]
        sorted_ids, _, status = _ssg_segments(points[order], _segments_of_sorted(b[order], n_samples), num_fps, radius)
        ids = torch.empty_like(sorted_ids)
        ids[order] = sorted_ids
    _fps.raise_on_status(status.item())
    return ids.to(batch_idx.dtype)


def _zyx_cells(points, batch_idx, cluster_vsize, point_cloud_range):
    """(sample, z, y, x) int64 cluster-voxel coordinates, as both assigners below form them (:1047-1051)"""
    dev = points.device
    cell = K.const_tensor(cluster_vsize, dev, points.dtype)
    origin = K.const_tensor(point_cloud_range[:3], dev, points.dtype)
    coors = torch.div(points - origin, cell, rounding_mode='floor').long()
    return torch.cat([batch_idx.long()[:, None], coors[:, [2, 1, 0]]], dim=1)


def _ssg_single_class(points, batch_idx, cells, num_fps, radius, per_sample):
    """cluster-voxel means -> ssg over them -> every point inherits its voxel's id; points whose voxel got none are
    dropped.  ONE read-back: the number of surviving points and the status word."""
    dev = points.device
    if points.size(0) == 0:
        return torch.zeros((0, 2), dtype=torch.long, device=dev), torch.zeros(0, dtype=torch.bool, device=dev)
    groups = K.unique_rows(cells.contiguous())
    voxels = K.segment_reduce(points.float().contiguous(), groups, 'mean')
    if per_sample:
        if groups.mins[0] < 0:
            raise RuntimeError('sst_amd: negative sample index')
        voxel_sample = K.unpack_unique_rows(groups, torch.int32)[:, 0]          # sorted-unique: sample after sample
        segments = _segments_of_sorted(voxel_sample, groups.mins[0] + groups.extents[0])
    else:
        segments = _one_segment(groups.m, dev)
    ids, _, status = _ssg_segments(voxels, segments, num_fps, radius)
    ids_per_point = ids[groups.inverse.long()]
    valid_pts_mask = ids_per_point > -1
    n_valid, status = torch.stack([valid_pts_mask.sum(), status[0].long()]).tolist()
    _fps.raise_on_status(status)
    keep = _nonzero_known(valid_pts_mask, n_valid)
    valid_pts_mask._sst_keep = keep
    return torch.stack([batch_idx.long()[keep], ids_per_point[keep].long()], 1), valid_pts_mask


class SSGAssigner(torch.nn.Module):
    """Furthest-point keypoints over the cluster-voxel means, pruned to non-overlapping balls; a point belongs to the one
    ball its voxel's mean falls in (single_stage_fsd.py:1002-1101; same constructor and forward).  As in the reference the
    sample index plays no part in sampling, pruning and assignment: ONE segment over all samples, the batch column only
    rides along in the output."""

    def __init__(self, cluster_voxel_size, point_cloud_range, radius, num_fps, class_names=['Car', 'Cyclist', 'Pedestrian']):
        super().__init__()
        self.cluster_voxel_size = cluster_voxel_size
        self.radius = radius
        self.num_fps = num_fps
        self.point_cloud_range = point_cloud_range
        self.class_names = class_names
        self.num_classes = len(class_names)

    _per_class = ClusterAssigner._per_class

    @torch.no_grad()
    def forward(self, points_list, batch_idx_list, gt_bboxes_3d=None, gt_labels_3d=None, origin_points=None):
        assert self.num_classes == len(self.class_names)
        outs = [self.forward_single_class(p, b, c, origin_points)
                for p, b, c in zip(points_list, batch_idx_list, self.class_names)]
        return modify_cluster_by_class([o[0] for o in outs]), [o[1] for o in outs]

    def forward_single_class(self, points, batch_idx, class_name, origin_points):
        cells = _zyx_cells(points, batch_idx, self._per_class(self.cluster_voxel_size, class_name), self.point_cloud_range)
        return _ssg_single_class(points, batch_idx, cells, self.num_fps[class_name], self._per_class(self.radius, class_name),
                                 per_sample=False)


class HybridAssigner(torch.nn.Module):
    """Per class either the ball assignment above, sample by sample (``assigner_type='ssg'``), or ClusterAssigner's
    connected components (``'ccl'``) (single_stage_fsd.py:1104-1194; same constructor and methods).  As in the reference
    both branches group by int64 (sample, z, y, x) coordinates and the ccl branch always labels per sample, whatever
    ``self.training`` says."""

    def __init__(self, point_cloud_range, cfg_per_class, class_names=['Car', 'Cyclist', 'Pedestrian']):
        super().__init__()
        self.point_cloud_range = point_cloud_range
        self.class_names = class_names
        self.cfg_per_class = cfg_per_class
        self.num_classes = len(class_names)

    @torch.no_grad()
    def forward(self, points_list, batch_idx_list, gt_bboxes_3d=None, gt_labels_3d=None, origin_points=None):
        assert self.num_classes == len(self.class_names)
        outs = [self.forward_single_class(p, b, c, origin_points)
                for p, b, c in zip(points_list, batch_idx_list, self.class_names)]
        return modify_cluster_by_class([o[0] for o in outs]), [o[1] for o in outs]

    def forward_single_class(self, points, batch_idx, class_name, origin_points):
        assigner_type = self.cfg_per_class[class_name]['assigner_type']
        if assigner_type == 'ssg':
            return self.forward_ssg(points, batch_idx, class_name, origin_points)
        elif assigner_type == 'ccl':
            return self.forward_ccl(points, batch_idx, class_name, origin_points)

    def forward_ssg(self, points, batch_idx, class_name, origin_points):
        cfg = self.cfg_per_class[class_name]
        cells = _zyx_cells(points, batch_idx, cfg['cluster_voxel_size'], self.point_cloud_range)
        return _ssg_single_class(points, batch_idx, cells, cfg['num_fps'], cfg['radius'], per_sample=True)

    def forward_ccl(self, points, batch_idx, class_name, origin_points):
        cfg = self.cfg_per_class[class_name]
        cells = _zyx_cells(points, batch_idx, cfg['cluster_voxel_size'], self.point_cloud_range)
        return _ccl_single_class(points, batch_idx.long(), cells, cfg['min_points'], cfg['connected_dist'], per_sample=True)
