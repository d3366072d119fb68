"""CTRL's offline stage: what the reference's tools/ctrl/ scripts compute before one training step can run, without their
per-pair and per-box host round trips.

- ``tracklet_affinity`` / ``generate_candidates`` / ``candidate_stats``: tools/ctrl/generate_candidates.py:39-78 (tracklet_assign
  with LiDARTracklet.max_iou per pair, stats) - every (predicted, ground-truth) pair of every segment in one launch and one host
  read; the lists are the ``candidates_list`` ``sst_amd.tracklet_targets`` consumes.
- ``box_point_crops`` / ``box_point_counts`` / ``crop_tracklet_points``: tools/ctrl/generate_track_input.py:88-101
  (extract_and_save_point: per frame and box points_in_boxes on the whole cloud, a mask, an index and a copy to the host) - a
  batch of frames in two launches and a scan, one host read (the total) in between.
- ``remove_empty_boxes``: tools/ctrl/remove_empty.py:82-134 (process_single_frame as shipped: box_grouping with group_size 1) -
  the count launch alone.

The work runs in csrc/tracklet_prep.hip behind the C ABI of include/sst_amd.h; there is no CPU path.  Reading and writing Waymo
``.bin`` files is not part of this library: the functions take tracklets and arrays.
"""
import ctypes
from collections import defaultdict

import numpy as np
import torch

from . import _lib
from .tracklet import _host_boxes, _pack

# tools/ctrl/remove_empty.py:155-160: the configuration the script ships per object type
REMOVE_EMPTY_DEFAULTS = {
    'vehicle': dict(bottom_lift=0.2, extra_hw=0.0, box_grouping=True, group_size=1),
    'pedestrian': dict(bottom_lift=0.1, extra_hw=0.0, box_grouping=True, group_size=1),
    'cyclist': dict(bottom_lift=0.1, extra_hw=0.0, box_grouping=True, group_size=1),
}

AFFINITY_ROW_BUDGET = 1 << 22      # box rows (predicted + ground truth) of one affinity launch
CROP_BYTE_BUDGET = 256 << 20       # bytes of points of one crop launch of crop_tracklet_points


def _device(device, tensors=()):
    if device is None:
        device = next((t.device for t in tensors if torch.is_tensor(t) and t.is_cuda), None)
        device = device if device is not None else torch.device('cuda', torch.cuda.current_device() if torch.cuda.is_available() else 0)
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('sst_amd: tracklet_prep needs a CUDA/HIP device (no CPU path in this library)')
    return dev


# ---- affinity and candidates ----------------------------------------------------------------------------------------------------

def _tracklet_boxes(trks, dev):
    """-> (host array [n, 7] or None, device tensor or None): one of the two"""
    host = [_host_boxes(t) for t in trks]
    if all(b is not None for b in host):
        return np.concatenate(host + [np.zeros((0, 7), np.float32)], 0), None
    if not trks:
        return np.zeros((0, 7), np.float32), None
    return None, torch.cat([t.boxes[:, :7].to(dev) for t in trks], 0).float().contiguous()


@torch.no_grad()
def _affinity_launch(pds, gts, ranges, dev):
    """the kernel on predicted tracklets ``pds``, ground-truth tracklets ``gts`` and per predicted tracklet the half-open range
    of ``gts`` it is paired with -> (affinity, out_offsets): the ragged device result and its host offsets"""
    for t in list(pds) + list(gts):
        if not getattr(t, 'frozen', False):
            raise RuntimeError('tracklet_affinity: tracklets must be frozen (freeze())')
        if t.boxes.dim() != 2 or t.boxes.size(1) != 7:
            raise RuntimeError(f'tracklet_affinity: boxes [n, 7] expected, got {tuple(t.boxes.shape)} (box widths other than 7 are not built)')
        if t.boxes.dtype != torch.float32:
            raise RuntimeError(f'tracklet_affinity: float32 boxes expected, got {t.boxes.dtype}')
    per_block = _lib.load().sst_tracklet_affinity_pairs_per_block()
    P = len(pds)
    begin = np.asarray([r[0] for r in ranges], np.int64).reshape(-1)
    end = np.asarray([r[1] for r in ranges], np.int64).reshape(-1)
    width = end - begin
    out_off = np.concatenate([[0], np.cumsum(width)]).astype(np.int64)
    blk_off = np.concatenate([[0], np.cumsum((width + per_block - 1) // per_block)]).astype(np.int64)
    pd_off = np.concatenate([[0], np.cumsum([len(t) for t in pds])]).astype(np.int64)
    gt_off = np.concatenate([[0], np.cumsum([len(t) for t in gts])]).astype(np.int64)
    pd_ts = np.asarray([x for t in pds for x in t.ts_list], np.int64).reshape(-1)
    gt_ts = np.asarray([x for t in gts for x in t.ts_list], np.int64).reshape(-1)
    n_out = int(out_off[-1])
    affinity = torch.empty(n_out, dtype=torch.float32, device=dev)
    if n_out == 0:
        return affinity, out_off
    hb_pd, db_pd = _tracklet_boxes(pds, dev)
    hb_gt, db_gt = _tracklet_boxes(gts, dev)
    floats = [b for b in (hb_pd, hb_gt) if b is not None]
    (d_pd_ts, d_pd_off, d_gt_ts, d_gt_off, d_begin, d_end, d_out_off, d_blk_off), d_floats = _pack(
        [pd_ts, pd_off, gt_ts, gt_off, begin, end, out_off, blk_off], floats, dev)
    d_floats = list(d_floats)
    pd_boxes = d_floats.pop(0) if hb_pd is not None else db_pd
    gt_boxes = d_floats.pop(0) if hb_gt is not None else db_gt
    a = _lib.TrackletAffinityArgs()
    a.pd_boxes, a.pd_ts, a.pd_offsets = pd_boxes.data_ptr(), d_pd_ts.data_ptr(), d_pd_off.data_ptr()
    a.gt_boxes, a.gt_ts, a.gt_offsets = gt_boxes.data_ptr(), d_gt_ts.data_ptr(), d_gt_off.data_ptr()
    a.pd_gt_begin, a.pd_gt_end = d_begin.data_ptr(), d_end.data_ptr()
    a.out_offsets, a.block_offsets, a.affinity = d_out_off.data_ptr(), d_blk_off.data_ptr(), affinity.data_ptr()
    a.n_pd_rows, a.n_gt_rows, a.n_pd, a.n_gt = int(pd_off[-1]), int(gt_off[-1]), P, len(gts)
    a.n_out, a.n_blocks = n_out, int(blk_off[-1])
    with torch.cuda.device(dev):
        _lib.check(_lib.load().sst_tracklet_affinity_f32(ctypes.byref(a), _lib.stream_ptr()), 'sst_tracklet_affinity_f32')
    return affinity, out_off


def tracklet_list2dict(tracklets):
    """tools/ctrl/generate_candidates.py:13-18 with the position of every tracklet in ``tracklets``: segment -> [index]"""
    out = defaultdict(list)
    for i, trk in enumerate(tracklets):
        out[trk.segment_name].append(i)
    return out


def tracklet_affinity(trks_pd, trks_gt, *, device=None, row_budget=AFFINITY_ROW_BUDGET):
    """``t_pd.max_iou(t_gt)`` for every predicted tracklet and every ground-truth tracklet of its segment
    (generate_candidates.py:61-62) -> a list over ``trks_pd`` of (gt_indices int64 array - positions in ``trks_gt``, in its order -,
    affinity float32 array).  A predicted tracklet whose segment has no ground truth gets two empty arrays.

    The tracklets are grouped by ``segment_name`` as tracklet_list2dict does; ``in_world`` must agree within every pair (max_iou
    asserts it).  Whole segments are gathered into launches of at most ``row_budget`` box rows (a single segment above the budget
    is one launch): per launch one packed copy to the device, one kernel, one read of the affinities."""
    dev = _device(device, [t.boxes for t in list(trks_pd) + list(trks_gt)])
    pd_of, gt_of = tracklet_list2dict(trks_pd), tracklet_list2dict(trks_gt)
    out = [None] * len(trks_pd)
    empty = (np.zeros(0, np.int64), np.zeros(0, np.float32))
    chunks, cur, rows = [], [], 0
    for seg, p_idx in pd_of.items():
        g_idx = gt_of.get(seg, [])
        if not g_idx:
            for i in p_idx:
                out[i] = empty
            continue
        worlds = {bool(trks_pd[i].in_world) for i in p_idx} | {bool(trks_gt[i].in_world) for i in g_idx}
        assert len(worlds) == 1, f'tracklet_affinity: in_world differs within segment {seg}'
        n = sum(len(trks_pd[i]) for i in p_idx) + sum(len(trks_gt[i]) for i in g_idx)
        if cur and rows + n > row_budget:
            chunks.append(cur)
            cur, rows = [], 0
        cur.append((p_idx, g_idx))
        rows += n
    if cur:
        chunks.append(cur)
    for chunk in chunks:
        pds, gts, ranges, where = [], [], [], []
        for p_idx, g_idx in chunk:
            g0 = len(gts)
            gts += [trks_gt[i] for i in g_idx]
            for i in p_idx:
                pds.append(trks_pd[i])
                ranges.append((g0, g0 + len(g_idx)))
                where.append((i, g_idx))
        aff, off = _affinity_launch(pds, gts, ranges, dev)
        aff = aff.cpu().numpy()
        for k, (i, g_idx) in enumerate(where):
            out[i] = (np.asarray(g_idx, np.int64), aff[off[k]:off[k + 1]])
    return out


def generate_candidates(trks_pd, trks_gt, affinity_thresh, *, device=None):
    """tracklet_assign + list_to_save of tools/ctrl/generate_candidates.py:39-66, :130 -> per predicted tracklet the list of the
    ground-truth tracklets (objects of ``trks_gt``, in its order) with ``affinity > affinity_thresh``: what the reference stores
    before ``to_dump_format``, and the ``candidates_list`` of ``sst_amd.tracklet_targets``.  A predicted tracklet whose segment has
    no ground truth is absent from the reference's dictionary and becomes ``[]``, as list_to_save does."""
    thresh = float(affinity_thresh)
    return [[trks_gt[int(g)] for g, v in zip(idx, aff) if float(v) > thresh]
            for idx, aff in tracklet_affinity(trks_pd, trks_gt, device=device)]


def candidate_stats(tracklets, candidates_list):
    """``stats`` of tools/ctrl/generate_candidates.py:71-77 -> (tracklet FP rate, box FP rate): the share of predicted tracklets,
    and of their boxes, without a candidate"""
    num_pred_boxes = sum(len(t) for t in tracklets)
    unmatched = [t for t, c in zip(tracklets, candidates_list) if len(c) == 0]
    return len(unmatched) / len(tracklets), sum(len(t) for t in unmatched) / num_pred_boxes


# ---- box modifications: a few torch operations on a [B, 7] tensor, on the host side of the call ---------------------------------------

def enlarged_box(boxes, extra_width):
    """LiDARInstance3DBoxes.enlarged_box (lidar_box3d.py:269-285) on a [B, 7] tensor"""
    out = boxes.clone()
    out[:, 3:6] += extra_width * 2
    out[:, 2] -= extra_width
    if extra_width < 0:
        invalid = (out[:, 3:6] <= 0).any(1)
        out[invalid] = boxes[invalid]
    return out


def enlarged_box_hw(boxes, extra_width):
    """LiDARInstance3DBoxes.enlarged_box_hw (lidar_box3d.py:331-346) on a [B, 7] tensor"""
    out = boxes.clone()
    out[:, 3:5] += extra_width * 2
    if extra_width < 0:
        invalid = (out[:, 3:5] <= 0).any(1)
        out[invalid] = boxes[invalid]
    return out


# ---- crops ----------------------------------------------------------------------------------------------------------------------

def _check_frames(points_list, boxes_list, what):
    if len(points_list) != len(boxes_list):
        raise RuntimeError(f'{what}: one box tensor per frame expected, got {len(points_list)} frames and {len(boxes_list)} box tensors')
    cols = None
    for p, b in zip(points_list, boxes_list):
        if p.dtype != torch.float32 or b.dtype != torch.float32:
            raise RuntimeError(f'{what}: float32 points and boxes expected, got {p.dtype} and {b.dtype}')
        if b.dim() != 2 or b.size(1) != 7:
            raise RuntimeError(f'{what}: boxes [B, 7] expected, got {tuple(b.shape)} (box widths other than 7 are not built)')
        if p.dim() != 2 or p.size(1) < 3:
            raise RuntimeError(f'{what}: points [N, C] with C >= 3 (xyz first) expected, got {tuple(p.shape)}')
        if cols is not None and p.size(1) != cols:
            raise RuntimeError(f'{what}: every frame must have the same number of point columns, got {cols} and {p.size(1)}')
        cols = p.size(1)
    _lib.require_cuda(*points_list, *boxes_list, contiguous=False)
    return cols


@torch.no_grad()
def _crops_packed(points, pt_lens, boxes, box_lens, fill):
    """points [sum N, C] and boxes [sum B, 7] on one device, frame after frame -> (rows, src, counts): the two launches and the scan;
    with fill = False the count launch alone (rows and src are None)"""
    lib = _lib.load()
    dev = points.device
    tile = lib.sst_box_crops_tile()
    F = len(pt_lens)
    pt_lens, box_lens = np.asarray(pt_lens, np.int64).reshape(-1), np.asarray(box_lens, np.int64).reshape(-1)
    tiles = (pt_lens + tile - 1) // tile
    cum = lambda v: np.concatenate([[0], np.cumsum(v)]).astype(np.int64)   # noqa: E731
    pt_off, box_off, tile_off, cell_off = cum(pt_lens), cum(box_lens), cum(tiles), cum(tiles * box_lens)
    n_points, n_boxes, n_tiles, n_cells = int(pt_off[-1]), int(box_off[-1]), int(tile_off[-1]), int(cell_off[-1])
    cols = points.size(1)
    counts = torch.empty(n_boxes, dtype=torch.int32, device=dev)
    (d_pt_off, d_box_off, d_tile_off, d_cell_off), _ = _pack([pt_off, box_off, tile_off, cell_off], [], dev)
    a = _lib.BoxCropsArgs()
    a.points, a.boxes, a.counts = points.data_ptr(), boxes.data_ptr(), counts.data_ptr()
    a.pt_offsets, a.box_offsets, a.tile_offsets, a.cell_offsets = (d_pt_off.data_ptr(), d_box_off.data_ptr(), d_tile_off.data_ptr(),
                                                                  d_cell_off.data_ptr())
    a.n_points, a.n_boxes, a.n_tiles, a.n_cells, a.n_frames, a.cols = n_points, n_boxes, n_tiles, n_cells, F, cols
    with torch.cuda.device(dev):
        if not fill:
            _lib.check(lib.sst_box_crops_count_f32(ctypes.byref(a), _lib.stream_ptr()), 'sst_box_crops_count_f32')
            return None, None, counts
        tile_counts = torch.zeros(max(n_cells, 1), dtype=torch.int32, device=dev)
        tile_starts = torch.empty(max(n_cells, 1), dtype=torch.int32, device=dev)
        total = torch.empty(1, dtype=torch.int32, device=dev)
        ws_bytes = int(lib.sst_box_crops_workspace_bytes(n_cells))
        ws = _lib.workspace(ws_bytes, dev)
        a.tile_counts, a.tile_starts, a.total = tile_counts.data_ptr(), tile_starts.data_ptr(), total.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
        _lib.check(lib.sst_box_crops_count_f32(ctypes.byref(a), _lib.stream_ptr()), 'sst_box_crops_count_f32')
        n_rows = int(total.item())                   # the one host read
        if n_rows < 0:
            raise RuntimeError('box_point_crops: more than 2^31 - 1 rows in one call; pass fewer frames')
        rows = torch.empty((n_rows, cols), dtype=torch.float32, device=dev)
        src = torch.empty(n_rows, dtype=torch.long, device=dev)
        a.rows, a.src, a.n_rows = rows.data_ptr(), src.data_ptr(), n_rows
        _lib.check(lib.sst_box_crops_fill_f32(ctypes.byref(a), _lib.stream_ptr()), 'sst_box_crops_fill_f32')
    return rows, src, counts


def _cat_frames(points_list, boxes_list, cols):
    dev = points_list[0].device if points_list else torch.device('cuda', torch.cuda.current_device())
    if points_list:
        points = points_list[0].contiguous() if len(points_list) == 1 else torch.cat(list(points_list), 0)
        boxes = boxes_list[0].contiguous() if len(boxes_list) == 1 else torch.cat(list(boxes_list), 0)
    else:
        points, boxes = torch.zeros((0, cols or 3), device=dev), torch.zeros((0, 7), device=dev)
    return points, boxes


def box_point_crops(points_list, boxes_list):
    """the points inside every box of every frame.  points_list: per frame [N_f, C] float32 device points (C >= 3, xyz first, the
    same C in every frame); boxes_list: per frame [B_f, 7] LiDAR boxes with a bottom centre ([x, y, z, w, l, h, ry]), already
    modified (``enlarged_box`` ..).  Every box is tested alone against every point of its frame with the inside test of
    ``sst_amd.points_in_boxes_batch``: a point may land in several boxes.

    -> (rows [sum counts, C], src int64 [sum counts] - the point's index in its frame -, counts int32 [sum B_f], offsets int64
    [sum B_f + 1]), all on the device; the rows of box b (boxes numbered frame after frame) are rows[offsets[b]:offsets[b + 1]],
    in ascending point index: ``pc[inbox_inds == 0]`` of generate_track_input.py:98-100.  One host read: the total."""
    cols = _check_frames(points_list, boxes_list, 'box_point_crops')
    points, boxes = _cat_frames(points_list, boxes_list, cols)
    rows, src, counts = _crops_packed(points, [p.size(0) for p in points_list], boxes, [b.size(0) for b in boxes_list], True)
    offsets = torch.zeros(counts.numel() + 1, dtype=torch.long, device=counts.device)
    torch.cumsum(counts, 0, out=offsets[1:])
    return rows, src, counts, offsets


def box_point_counts(points_list, boxes_list):
    """the number of points inside every box of every frame (the arguments of ``box_point_crops``) -> counts int32 [sum B_f] on the
    device: the first launch alone, nothing read back"""
    cols = _check_frames(points_list, boxes_list, 'box_point_counts')
    points, boxes = _cat_frames(points_list, boxes_list, cols)
    return _crops_packed(points, [p.size(0) for p in points_list], boxes, [b.size(0) for b in boxes_list], False)[2]


def crop_tracklet_points(tracklets, frames, extra_width, *, device=None, byte_budget=CROP_BYTE_BUDGET):
    """extract_and_save_point of tools/ctrl/generate_track_input.py:69-114 for the tracklets of ONE segment.

    tracklets: frozen LiDARTracklet of the segment; frames: a mapping timestamp -> points [N, C] (float32 array or tensor, xyz
    first) of the segment's frames, walked in ascending timestamp and consumed in chunks of at most ``byte_budget`` bytes of
    points (a single larger frame is its own chunk): per chunk one copy to the device, two launches, one read of the total and
    one of the crops.  Every box is enlarged by ``extra_width`` (``enlarged_box``) on the host.

    -> the ``pc_list`` of every tracklet: one [n, C] float32 array per frame of its ``ts_list`` that ``frames`` holds (a frame
    without a box of the tracklet is skipped, as ``trk[ts] is None`` is); every timestamp of a tracklet must be in ``frames``
    (the reference's append_pc asserts that order).  Sets ``num_pts_in_boxes`` of every tracklet."""
    dev = _device(device)
    for t in tracklets:
        if not getattr(t, 'frozen', False):
            raise RuntimeError('crop_tracklet_points: tracklets must be frozen (freeze())')
        if t.boxes.size(0) and t.boxes.size(1) != 7:
            raise RuntimeError(f'crop_tracklet_points: boxes [n, 7] expected, got {tuple(t.boxes.shape)} (box widths other than 7 are not built)')
        if t.boxes.dtype != torch.float32:
            raise RuntimeError(f'crop_tracklet_points: float32 boxes expected, got {t.boxes.dtype}')
    pc_lists = [[] for _ in tracklets]
    chunk, nbytes = [], 0

    def flush():
        if not chunk:
            return
        pts_np = [p for _, p, _, _ in chunk]
        cols = pts_np[0].shape[1]
        points = torch.from_numpy(np.concatenate(pts_np, 0)).to(dev)
        boxes = torch.cat([b for _, _, b, _ in chunk], 0).to(dev)
        rows, _, counts = _crops_packed(points, [len(p) for p in pts_np], boxes, [b.size(0) for _, _, b, _ in chunk], True)
        rows, counts = rows.cpu().numpy(), counts.cpu().numpy().astype(np.int64)
        off = np.concatenate([[0], np.cumsum(counts)])
        k = 0
        for ts, _, _, owners in chunk:
            for i in owners:
                t = tracklets[i]
                assert ts == t.ts_list[len(pc_lists[i])], 'crop_tracklet_points: a timestamp of a tracklet is missing from frames'
                pc_lists[i].append(rows[off[k]:off[k + 1]].reshape(-1, cols))
                k += 1
        chunk.clear()

    cols = None
    for ts in sorted(frames):
        pc = frames[ts]
        pc = pc.detach().cpu().numpy() if torch.is_tensor(pc) else np.asarray(pc)
        if pc.dtype != np.float32:
            raise RuntimeError(f'crop_tracklet_points: float32 points expected, got {pc.dtype}')
        if pc.ndim != 2 or pc.shape[1] < 3:
            raise RuntimeError(f'crop_tracklet_points: points [N, C] with C >= 3 (xyz first) expected, got {pc.shape}')
        if cols is not None and pc.shape[1] != cols:
            raise RuntimeError(f'crop_tracklet_points: every frame must have the same number of point columns, got {cols} and {pc.shape[1]}')
        cols = pc.shape[1]
        owners = [i for i, t in enumerate(tracklets) if t.ts2index.get(ts) is not None]
        if not owners:
            continue
        boxes = torch.cat([tracklets[i][ts].detach().cpu() for i in owners], 0)
        if chunk and nbytes + pc.nbytes > byte_budget:
            flush()
            nbytes = 0
        chunk.append((ts, np.ascontiguousarray(pc), enlarged_box(boxes, extra_width), owners))
        nbytes += pc.nbytes
    flush()
    for t, pcs in zip(tracklets, pc_lists):
        t.num_pts_in_boxes = [len(p) for p in pcs]
    return pc_lists


def remove_empty_boxes(boxes_list, points_list, bottom_lift, extra_hw=None, *, box_grouping=True, group_size=1,
                       origin=(0.5, 0.5, 0.5)):
    """the keep masks of process_single_frame of tools/ctrl/remove_empty.py:65-113 as the script ships it (``box_grouping`` with
    ``group_size`` 1, REMOVE_EMPTY_DEFAULTS per object type): a box is kept when it holds at least one point of its frame.

    boxes_list: per frame [B_f, 7] float32 device boxes as the script reads them - centred at ``origin`` of the box ((0.5, 0.5,
    0.5): the gravity centre of a Waymo label; pass (0.5, 0.5, 0) for bottom-centred boxes); the constructor's shift to the bottom
    centre, ``z += h * bottom_lift`` and ``enlarged_box_hw(extra_hw)`` are applied here.  points_list: per frame [N_f, C >= 3].

    -> (masks, dropped): per frame a bool array [B_f], and per frame whether NO box of it holds a point.  Without box_grouping the
    reference drops such a frame whole (``continue`` at :94-95: it never reaches the output list); with box_grouping, as shipped,
    the frame stays with an all-False mask.  The caller decides; this function only reports the fact.  One launch, one read."""
    if not box_grouping:
        raise NotImplementedError('remove_empty_boxes: box_grouping=False (first-match points_in_boxes over all boxes of a frame) is '
                                  'not built; the shipped configurations set box_grouping=True, group_size=1')
    if group_size != 1:
        raise NotImplementedError(f'remove_empty_boxes: box_grouping with group_size={group_size} is not built (it needs the '
                                  f'first-match rule over a random permutation); the shipped configurations set group_size=1')
    cols = _check_frames(points_list, boxes_list, 'remove_empty_boxes')
    moved = []
    for b in boxes_list:
        b = b.clone()
        if tuple(origin) != (0.5, 0.5, 0):
            b[:, :3] += b[:, 3:6] * (b.new_tensor((0.5, 0.5, 0)) - b.new_tensor(tuple(origin)))
        b[:, 2] += b[:, 5] * bottom_lift
        if extra_hw is not None:
            b = enlarged_box_hw(b, extra_hw)
        moved.append(b)
    points, boxes = _cat_frames(points_list, moved, cols)
    counts = _crops_packed(points, [p.size(0) for p in points_list], boxes, [b.size(0) for b in moved], False)[2].cpu().numpy()
    masks, k = [], 0
    for b in moved:
        masks.append(counts[k:k + b.size(0)] > 0)
        k += b.size(0)
    return masks, [not bool(m.any()) for m in masks]
