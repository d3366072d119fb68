"""The tracklet training targets (csrc/tracklet.hip, sst_amd/tracklet.py) restated in torch the way the reference computes them -
tracklet by tracklet, candidate by candidate, with its host reads - in float32 or float64, on the CPU or (with the library's
aligned IoU) on the device: for tests/test_tracklet_host.py, tests/test_gpu_tracklet.py, tests/golden/make_tracklet.py and
tools/tracklet_bench.py.

- aligned_iou: LiDARInstance3DBoxes.aligned_iou_3d with the BEV overlap of tests/box_ops_ref.py (float32: the reference's polygon
  algorithm operation by operation with the library's cap; float64: an independent clip).
- targets: _select_one2one_candidates (the first candidate with the most shared timestamps of IoU > candidate_thresh),
  TrackletAssigner.assign, PseudoSampler's order (positives in frame order, then negatives) and get_targets in that order, in the
  row layout of sst_amd.tracklet_targets.  ``stats`` counts the IoU launches and the host reads the reference's code makes.
- rows: the gathers and cats in front of the box head (tracklet_roi_head.py:247-258) by torch indexing.
"""
import numpy as np
import torch

import box_ops_ref as B
import roi_head_ref as R


def aligned_iou(a, b, dtype=torch.float32):
    """[N, 7] x [N, 7] CPU tensors -> [N] aligned 3-D IoU in ``dtype``"""
    npdt = np.float32 if dtype == torch.float32 else np.float64
    a, b = np.asarray(a)[:, :7].astype(npdt), np.asarray(b)[:, :7].astype(npdt)
    if len(a) == 0:
        return torch.zeros(0, dtype=dtype)
    ra, rb = R.bev_rows(a), R.bev_rows(b)
    if npdt == np.float32:
        bev = B.bev_overlap_f32(ra, rb)
        bev = np.minimum(bev, np.minimum(np.abs((ra[:, 2] - ra[:, 0]) * (ra[:, 3] - ra[:, 1])),
                                         np.abs((rb[:, 2] - rb[:, 0]) * (rb[:, 3] - rb[:, 1])))).astype(np.float32)
    else:
        bev = np.array([B.bev_overlap_f64(x, y) for x, y in zip(ra, rb)], np.float64).reshape(-1)
    oh = np.maximum(np.minimum(a[:, 2] + a[:, 5], b[:, 2] + b[:, 5]) - np.maximum(a[:, 2], b[:, 2]), npdt(0))
    o3 = bev * oh
    v1, v2 = a[:, 3] * a[:, 4] * a[:, 5], b[:, 3] * b[:, 4] * b[:, 5]
    return torch.as_tensor((o3 / np.maximum(v1 + v2 - o3, npdt(1e-8))).astype(npdt))


def per_class(value, n):
    return [float(v) for v in value] if isinstance(value, (list, tuple)) else [float(value)] * n


def targets(tracklets, candidates_list, cfg, dtype=torch.float32, iou_fn=None, class_indices=None, stats=None):
    """tracklets / candidates: objects with ``boxes`` [n, 7] tensor, ``ts_list``, ``score_list``, ``type``.  cfg: candidate_thresh,
    object_centric, iou_thr, cls_pos_thr, cls_neg_thr, num_classes.  iou_fn(boxes1, boxes2) -> [N] (default: aligned_iou in
    ``dtype`` on the CPU)."""
    iou_fn = iou_fn or (lambda x, y: aligned_iou(x.cpu(), y.cpu(), dtype))
    stats = stats if stats is not None else {}
    stats.setdefault('iou_launches', 0)
    stats.setdefault('host_reads', 0)
    nc = cfg.get('num_classes', 3)
    cpos, cneg = per_class(cfg['cls_pos_thr'], nc), per_class(cfg['cls_neg_thr'], nc)
    thresh = cfg.get('candidate_thresh', 0.5)
    out = {k: [] for k in ('rois', 'src', 'gt_index', 'labels', 'iou', 'soft_label', 'reg_mask', 'targets', 'frame_inds', 'scores',
                           'pos_gt_bboxes', 'matched', 'overlaps', 'assigned_gt_inds', 'chosen', 'counts')}
    r0 = g0 = 0
    for t, (trk, cands) in enumerate(zip(tracklets, candidates_list)):
        dev = trk.boxes.device
        boxes = trk.boxes[:, :7].to(dtype)
        n = len(trk.ts_list)
        index_of = {ts: i for i, ts in enumerate(trk.ts_list)}

        def shared(c):
            inter = sorted(set(trk.ts_list) & set(c.ts_list))
            c_index = {ts: i for i, ts in enumerate(c.ts_list)}
            return ([index_of[ts] for ts in inter], [c_index[ts] for ts in inter])

        def inter_ious(c):
            i1, i2 = shared(c)
            if not i1:
                return boxes.new_zeros(0), i1, i2
            stats['iou_launches'] += 1
            return (iou_fn(boxes[torch.tensor(i1, device=dev)], c.boxes[:, :7].to(dtype)[torch.tensor(i2, device=dev)]).to(dtype),
                    i1, i2)

        # _select_one2one_candidates: a host tensor of the counts, torch.argmax, .item()
        chosen = -1
        if len(cands):
            aff = []
            for c in cands:
                aff.append((inter_ious(c)[0] > thresh).sum().cpu())
                stats['host_reads'] += 1
            chosen = int(torch.argmax(torch.tensor(aff)).item())
        gt = cands[chosen] if chosen >= 0 else None
        m = len(gt.ts_list) if gt is not None else 0
        # TrackletAssigner.assign
        overlaps = boxes.new_zeros(n)
        matched = torch.full((n,), -1, dtype=torch.long)
        if m and n:
            ious, i1, i2 = inter_ious(gt)
            if i1:
                overlaps[torch.tensor(i1, device=dev)] = ious
                matched[torch.tensor(i1)] = torch.tensor(i2)
            if cfg.get('object_centric', False):
                ov = overlaps.tolist()            # the reference reads overlaps[i].item() per box
                stats['host_reads'] += n
                assigned = torch.tensor([int(matched[i]) + 1 if ov[i] > cfg.get('iou_thr', 0.5) else 0 for i in range(n)])
            else:
                assigned = matched + 1
        else:
            assigned = torch.zeros(n, dtype=torch.long)
        # PseudoSampler
        pos_inds = torch.nonzero(assigned > 0, as_tuple=False).reshape(-1)
        neg_inds = torch.nonzero(assigned == 0, as_tuple=False).reshape(-1)
        stats['host_reads'] += 2                  # the two nonzero calls
        order = torch.cat([pos_inds, neg_inds])
        n_pos = len(pos_inds)
        cls = int(trk.type if class_indices is None else class_indices[t])
        order_d = order.to(dev)
        rois = torch.cat([boxes.new_full((n, 1), t), boxes[order_d]], 1)
        iou = overlaps[order_d]
        gt_local = assigned[pos_inds] - 1
        gt_boxes = gt.boxes[:, :7].to(dtype)[gt_local.to(dev)] if n_pos else boxes.new_zeros((0, 7))
        tg = boxes.new_zeros((n, 7))
        pgb = boxes.new_zeros((n, 7))
        soft = boxes.new_zeros(n)
        if n_pos:
            tg[:n_pos] = R.target_rows(boxes[order_d[:n_pos]], gt_boxes, dtype)
            pgb[:n_pos] = gt_boxes
            # on the host: the device divides by a Python scalar through its reciprocal, the host divides
            p_iou = iou[:n_pos].cpu()
            pos_m, neg_m = p_iou > cpos[cls], p_iou < cneg[cls]
            lab = pos_m.to(dtype)
            mid = ~pos_m & ~neg_m
            lab[mid] = (p_iou[mid] - cneg[cls]) / (cpos[cls] - cneg[cls])
            soft[:n_pos] = lab.to(dev)
        cand_base = g0 + sum(len(c.ts_list) for c in cands[:max(chosen, 0)])
        out['rois'].append(rois.cpu())
        out['src'].append((order + r0).to(torch.int32))
        out['gt_index'].append(torch.cat([gt_local + cand_base, torch.full((n - n_pos,), -1)]).to(torch.int32))
        out['labels'].append(torch.cat([torch.full((n_pos,), cls), torch.full((n - n_pos,), -1)]).long())
        out['iou'].append(iou.cpu())
        out['soft_label'].append(soft.cpu())
        out['reg_mask'].append(torch.cat([torch.ones(n_pos), torch.zeros(n - n_pos)]).to(torch.uint8))
        out['targets'].append(tg.cpu())
        out['frame_inds'].append(order)
        out['scores'].append(torch.tensor(trk.score_list, dtype=torch.float32).reshape(-1)[order])
        out['pos_gt_bboxes'].append(pgb.cpu())
        out['matched'].append(matched.to(torch.int32))
        out['overlaps'].append(overlaps.cpu())
        out['assigned_gt_inds'].append(assigned.long())
        out['chosen'].append(chosen)
        out['counts'].append((n_pos, n - n_pos))
        r0 += n
        g0 += sum(len(c.ts_list) for c in cands)
    res = {k: torch.cat(v) for k, v in out.items() if k not in ('chosen', 'counts')}
    res['chosen'] = torch.tensor(out['chosen'], dtype=torch.int32)
    res['counts'] = torch.tensor(out['counts'], dtype=torch.int32).reshape(-1, 2)
    return res


def rows(pts_feats, pts_xyz, pts_frame_inds, ext_pts_inds, ext_pts_roi_inds, roi_frame_inds, roi_scores, combined, with_roi_scores):
    """tracklet_roi_head.py:247-258 by torch indexing and cat -> (new_pts_feats, new_pts_xyz)"""
    new_pts_feats = pts_feats[ext_pts_inds]
    new_pts_xyz = pts_xyz[ext_pts_inds]
    if combined:
        is_cur_frame = (pts_frame_inds[ext_pts_inds] == roi_frame_inds[ext_pts_roi_inds]).to(new_pts_feats.dtype)
        new_pts_feats = torch.cat([new_pts_feats, is_cur_frame.unsqueeze(1)], 1)
    if with_roi_scores:
        new_pts_feats = torch.cat([new_pts_feats, roi_scores[ext_pts_roi_inds].to(new_pts_feats.dtype).unsqueeze(1)], 1)
    return new_pts_feats, new_pts_xyz


def rows_grad(d_out, ext_pts_inds, n, f, dtype=torch.float64):
    """the gradient of pts_feats: per source point the sum of its output rows in ascending row order, in ``dtype``"""
    p = torch.where(ext_pts_inds < 0, ext_pts_inds + n, ext_pts_inds)
    g = torch.zeros((n, f), dtype=dtype)
    d = d_out[:, :f].to(dtype)
    for i in range(len(p)):                       # ascending output row: the one order of the additions
        g[p[i]] += d[i]
    return g


# ---- scenes ------------------------------------------------------------------------------------------------------------------

class Trk(object):
    """the fields of a tracklet the restatement reads"""

    def __init__(self, boxes, ts_list, score_list, type_):
        self.boxes, self.ts_list, self.score_list, self.type = torch.as_tensor(boxes, dtype=torch.float32), list(ts_list), list(score_list), type_


TS0 = 1_550_000_000_000_000


def track_boxes(rng, n, kind):
    """n boxes of one object moving along a gently turning path; kind 0 car, 1 pedestrian, 2 cyclist"""
    size = [(2.0, 4.6, 1.7), (0.8, 0.9, 1.75), (0.8, 1.8, 1.7)][kind]
    yaw0 = rng.uniform(-np.pi, np.pi)
    yaw = yaw0 + np.cumsum(rng.normal(0, 0.01, n))
    step = rng.uniform(0.05, 0.6)
    # the yaw of a LiDAR box of this convention is measured from the y axis towards x: heading (sin, cos)
    xy = rng.uniform(-30, 30, 2) + np.cumsum(np.stack([np.sin(yaw), np.cos(yaw)], 1) * step, 0)
    z = rng.uniform(-1.5, 0.5) + rng.normal(0, 0.02, n)
    wlh = np.asarray(size)[None] * (1 + rng.normal(0, 0.02, (n, 3)))
    return np.concatenate([xy, z[:, None], wlh, yaw[:, None]], 1).astype(np.float32)


def jitter(rng, boxes, scale):
    noise = rng.normal(0, 1, boxes.shape) * np.array([0.25, 0.25, 0.08, 0.06, 0.12, 0.05, 0.06]) * scale
    out = (boxes + noise).astype(np.float32)
    out[:, 3:6] = np.maximum(out[:, 3:6], 0.2)
    return out


def make_tracklets(seed, lens, n_cands, kinds=None, gt_stride=1):
    """-> (tracklets, candidates_list): per tracklet a ground-truth path, the prediction = its jittered boxes (yaw of either sense
    now and then), candidates = the path itself on a subset of the frames (+ frames outside the tracklet), weaker copies of it,
    and one that shares no timestamp"""
    rng = np.random.default_rng(seed)
    trks, cand_lists = [], []
    for t, n in enumerate(lens):
        kind = (t % 3) if kinds is None else kinds[t]
        ts = [TS0 + 100_000 * (7 * t + i) for i in range(n)]
        path = track_boxes(rng, n + 6, kind)
        scale = rng.choice([0.3, 1.0, 2.5], n)[:, None]
        pred = jitter(rng, path[:n], scale)
        flip = rng.random(n) < 0.15
        pred[flip, 6] += np.float32(np.pi)
        trks.append(Trk(pred, ts, rng.uniform(0.1, 0.95, n).astype(np.float32).tolist(), kind))
        cands = []
        for c in range(n_cands[t]):
            if c % 4 == 3:        # shares no timestamp
                cts = [x + 50_000 for x in ts[:max(n // 2, 1)]]
                cb = path[:len(cts)]
            else:
                keep = np.nonzero((rng.random(n) < (0.9 if c == 0 else 0.6)) | (np.arange(n) == (c % max(n, 1))))[0][::gt_stride]
                extra = list(range(n, min(n + 3 + c, n + 6)))      # timestamps outside the tracklet
                cts = [ts[i] for i in keep] + [TS0 + 100_000 * (7 * t + i) for i in extra]
                cb = np.concatenate([path[keep], path[extra]], 0)
                if c > 0:
                    cb = jitter(rng, cb, 1.5 * c)
            cands.append(Trk(cb.copy(), cts, [1.0] * len(cts), kind))
        cand_lists.append(cands)
    return trks, cand_lists


def gold_scene(g):
    """the batch of tests/golden/tracklet_train.npz -> (tracklets, candidates_list) of Trk"""
    trks, cand_lists = [], []
    r0 = c0 = g0 = 0
    for t, n in enumerate(g['lens'].tolist()):
        trks.append(Trk(g['boxes'][r0:r0 + n], g['ts'][r0:r0 + n].tolist(), g['scores'][r0:r0 + n].tolist(), int(g['kinds'][t])))
        cands = []
        for m in g['cand_lens'][c0:c0 + int(g['n_cands'][t])].tolist():
            cands.append(Trk(g['cand_boxes'][g0:g0 + m], g['cand_ts'][g0:g0 + m].tolist(), [1.0] * m, int(g['kinds'][t])))
            g0 += m
        cand_lists.append(cands)
        r0, c0 = r0 + n, c0 + int(g['n_cands'][t])
    return trks, cand_lists


GOLD_CFG = dict(candidate_thresh=0.5, iou_thr=0.45, cls_pos_thr=(0.8, 0.65, 0.7), cls_neg_thr=(0.2, 0.15, 0.25), num_classes=3)


def bar(gap):
    """the tolerance of the heads' tests: max(4 x the reference's own float32-vs-float64 gap, 1e-6), relative to the largest element"""
    return max(4 * float(gap), 1e-6)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if b.size else 0.0
