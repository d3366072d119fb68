"""Generates tests/golden/tracklet_train.npz: the tracklet training targets, the RoIs of tracklets, the decoded boxes and the host
methods of LiDARTracklet as the REFERENCE computes them (data only).

Needs the reference tree (oracle.ref_loader); run from the repository root:  python tests/golden/make_tracklet.py

Executed from their source text: LiDARTracklet (core/bbox/structures/lidar_tracklet.py), TrackletAssigner
(core/bbox/assigners/tracklet_assigner.py), TrackletRoIHead._select_one2one_candidates / _assign_and_sample / tracklets2rois /
get_gt_rois (roi_heads/tracklet_roi_head.py), FullySparseBboxHead.get_targets / _get_target_single / get_multi_class_soft_label
/ get_class_wise_box_weights / decode_from_rois / get_bboxes_from_tracklet (bbox_heads/fsd_bbox_head.py), LiDARInstance3DBoxes
with aligned_iou_3d, flip, rotate, translate, scale and heading_unit_vector (structures/lidar_box3d.py, base_box3d.py) and
DeltaXYZWLHRBBoxCoder - loaded as tests/golden/make_roi_head_train.py loads them; and the state_dict key lists of the three
shipped CTRL configs (reference_state_keys below).  Stand-ins for what the reference imports
from packages that are not in its tree, or runs on CUDA only:
  mmdet PseudoSampler           as mmdet 2.x has it: pos_inds = nonzero(gt_inds > 0), neg_inds = nonzero(gt_inds == 0), both
                                unique (ascending), every box kept
  mmdet SamplingResult          the fields of mmdet 2.x, including its view of an empty ground truth as [0, 4] - the shape
                                TrackletRoIHead's hack_sampler_bug turns into [0, 7]
  mmdet AssignResult, BaseAssigner            a plain record, object
  TorchEx boxes_overlap_1to1    the diagonal of tests/box_ops_ref.py (float32: the reference's polygon algorithm operation by
                                operation; float64: an independent clip)
  bbox3d2roi, multi_apply       the sample index as column 0; map / zip
Every case runs in float32 and in float64 (the same source text with ``torch.float32`` read as ``torch.float64`` and
``Tensor.float()`` as ``Tensor.double()``); noise_* is the gap between the two runs.  The predicted boxes are re-drawn until, in
float64, no IoU of a shared timestamp lies within max(1e-4, 10 noise_iou) of candidate_thresh, iou_thr, cls_pos_thr or
cls_neg_thr, and no canonical yaw within 0.05 rad of pi / 2, pi or 3 pi / 2.

The batch, eight tracklets: lengths 1, 63, 64, 65, 200, 12, 30, 17; 1, 0, 3, 3, 3, 1, 2, 3 candidates; tracklet 3's first two
candidates are identical (tied on the count: the first wins); tracklet 5's only candidate shares no timestamp (chosen, but no
positive); tracklet 1 has no candidate (the empty ground truth, the hack_sampler_bug shape); candidates carry timestamps outside
their tracklet; the best candidate of tracklet 4 is its last, of tracklet 7 its middle one; the classes 0 / 1 / 2 have different thresholds; everything is run with object_centric on and off.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'tests'), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import box_ops_ref as B  # noqa: E402
import roi_head_ref as R  # noqa: E402
import tracklet_ref as T  # noqa: E402
import make_roi_head_train as M  # noqa: E402

TRK_PY = 'mmdet3d/core/bbox/structures/lidar_tracklet.py'
ASSIGNER_PY = 'mmdet3d/core/bbox/assigners/tracklet_assigner.py'
ROI_PY = 'mmdet3d/models/roi_heads/tracklet_roi_head.py'
LENS = [1, 63, 64, 65, 200, 12, 30, 17]
N_CANDS = [1, 0, 3, 3, 3, 1, 2, 3]
KINDS = [0, 1, 2, 0, 0, 1, 2, 1]
CFG = dict(candidate_thresh=0.5, iou_thr=0.45, cls_pos_thr=(0.8, 0.65, 0.7), cls_neg_thr=(0.2, 0.15, 0.25), num_classes=3)
THRESHOLDS = (0.5, 0.45, 0.8, 0.65, 0.7, 0.2, 0.15, 0.25)


class TorchAsFloat64(object):
    """``torch`` for the float64 run: float32 and float read as float64"""

    def __getattr__(self, name):
        return torch.float64 if name in ('float32', 'float') else getattr(torch, name)


class SamplingResult(M.SamplingResult):
    def __init__(self, pos_inds, neg_inds, bboxes, gt_bboxes, assign_result, gt_flags):
        super().__init__(pos_inds, neg_inds, bboxes, gt_bboxes, assign_result, gt_flags)
        if gt_bboxes.numel() == 0:
            self.pos_gt_bboxes = torch.empty_like(gt_bboxes).view(-1, 4)


class PseudoSampler(object):
    def sample(self, assign_result, bboxes, gt_bboxes, **kwargs):
        pos_inds = torch.nonzero(assign_result.gt_inds > 0, as_tuple=False).squeeze(-1).unique()
        neg_inds = torch.nonzero(assign_result.gt_inds == 0, as_tuple=False).squeeze(-1).unique()
        gt_flags = bboxes.new_zeros(bboxes.shape[0], dtype=torch.uint8)
        return SamplingResult(pos_inds, neg_inds, bboxes, gt_bboxes, assign_result, gt_flags)


def reference_parts(f64):
    from oracle import ref_loader as L
    parts = M.reference_parts(f64)
    tm = TorchAsFloat64() if f64 else torch
    npdt = np.float64 if f64 else np.float32
    lidar = parts['lidar']

    def boxes_overlap_1to1(a, b):
        ra, rb = a.numpy().astype(npdt), b.numpy().astype(npdt)
        if f64:
            return torch.as_tensor(np.array([B.bev_overlap_f64(x, y) for x, y in zip(ra, rb)], np.float64).reshape(-1))
        return torch.as_tensor(B.bev_overlap_f32(ra, rb).astype(np.float32))

    lidar.aligned_iou_3d.__func__.__globals__['boxes_overlap_1to1'] = boxes_overlap_1to1
    import copy
    import torch.nn.functional as F
    parts['tracklet'] = L.load_reference_class(TRK_PY, 'LiDARTracklet', dict(np=np, torch=tm, F=F, LiDARInstance3DBoxes=lidar, copy=copy))
    parts['assigner'] = L.load_reference_class(ASSIGNER_PY, 'TrackletAssigner', dict(torch=tm, BaseAssigner=object,
                                                                                     AssignResult=M.AssignResult))
    glb = dict(torch=tm, PseudoSampler=PseudoSampler, bbox3d2roi=M.bbox3d2roi, LiDARInstance3DBoxes=lidar)
    parts['roi_methods'] = {k: L.load_reference_method(ROI_PY, 'TrackletRoIHead', k, glb)
                            for k in ('_select_one2one_candidates', '_assign_and_sample', 'tracklets2rois', 'get_gt_rois')}
    hglb = parts['methods']['get_targets'].__globals__
    for k in ('decode_from_rois', 'get_bboxes_from_tracklet'):
        parts['methods'][k] = L.load_reference_method(M.HEAD_PY, 'FullySparseBboxHead', k, dict(hglb))
    return parts


def ref_tracklet(parts, trk, name):
    boxes = trk.boxes.numpy().astype(np.float32)
    t = parts['tracklet']('seg', name, int(trk.type), True, [boxes[i:i + 1] for i in range(len(boxes))], list(trk.ts_list),
                          [float(s) for s in trk.score_list])
    if len(boxes):
        t.freeze()
    else:                       # freeze() reads box_list[0]; what it sets otherwise
        t.ts2index, t.ts_set, t.frozen, t.size = {}, set(), True, 0
        t.device, t.dtype = torch.device('cpu'), parts['dtype']
    t.set_type(int(trk.type), 'mmdet3d')
    t.type_name = M.R.WAYMO_NAMES[int(trk.type)]      # set by the reference's dataset
    return t


def make_roi_head(parts, object_centric):
    head = types.SimpleNamespace(train_cfg=M.Cfg(candidate_thresh=CFG['candidate_thresh'], hack_sampler_bug=True),
                                 bbox_assigner=parts['assigner'](object_centric=object_centric, iou_thr=CFG['iou_thr']),
                                 bbox_sampler=PseudoSampler())
    for k, fn in parts['roi_methods'].items():
        setattr(head, k, types.MethodType(fn, head))
    return head


def make_bbox_head(parts, test_cfg=None):
    head = types.SimpleNamespace(num_classes=3, bbox_coder=parts['coder'](), test_cfg=M.Cfg(test_cfg or {}),
                                 train_cfg=M.Cfg(cls_pos_thr=CFG['cls_pos_thr'], cls_neg_thr=CFG['cls_neg_thr']))
    for k, fn in parts['methods'].items():
        setattr(head, k, types.MethodType(fn, head))
    return head


def run_targets(parts, trks, cand_lists, object_centric):
    f64 = parts['dtype'] == torch.float64
    with M.patched(f64):
        rt = [ref_tracklet(parts, t, f'p{i}') for i, t in enumerate(trks)]
        rc = [[ref_tracklet(parts, c, f'c{i}_{j}') for j, c in enumerate(cs)] for i, cs in enumerate(cand_lists)]
        roi_head = make_roi_head(parts, object_centric)
        chosen_trks = roi_head._select_one2one_candidates(rt, rc)
        chosen = [next((j for j, c in enumerate(cs) if c is g), -1) for cs, g in zip(rc, chosen_trks)]
        results = roi_head._assign_and_sample(rt, rc)
        assigned = [roi_head.bbox_assigner.assign(a, g).gt_inds.numpy() for a, g in zip(rt, chosen_trks)]
        bbox_head = make_bbox_head(parts)
        label, bbox_targets, _, pos_gt_bboxes, pos_gt_labels, reg_mask = bbox_head.get_targets(results, bbox_head.train_cfg)[:6]
        rois, roi_frame_inds, cls_preds, labels_3d = roi_head.tracklets2rois(rt)
        gt_rois = roi_head.get_gt_rois(rt, chosen_trks)
    mask = reg_mask.numpy() == 1
    full = np.zeros((len(mask), 7), np.float64)
    full[mask] = bbox_targets.numpy()
    pgb = np.zeros((len(mask), 7), np.float64)
    pgb[mask] = pos_gt_bboxes.numpy()
    labels = np.full(len(mask), -1, np.int64)
    labels[mask] = pos_gt_labels.numpy()
    return dict(chosen=np.asarray(chosen, np.int32), assigned_gt_inds=np.concatenate(assigned).astype(np.int64),
                frame_inds=torch.cat([r.bboxes_frame_inds for r in results]).numpy().astype(np.int64),
                counts=np.asarray([(len(r.pos_inds), len(r.neg_inds)) for r in results], np.int32), reg_mask=mask.astype(np.uint8),
                labels=labels, iou=torch.cat([r.iou for r in results]).numpy(), scores=torch.cat([r.scores for r in results]).numpy(),
                soft_label=label.numpy(), targets=full, pos_gt_bboxes=pgb, sampled_rois=M.bbox3d2roi([r.bboxes for r in results]).numpy(),
                rois=rois.numpy(), roi_frame_inds=roi_frame_inds.numpy(), cls_preds=cls_preds.numpy(), labels_3d=labels_3d.numpy(),
                gt_rois=gt_rois.numpy())


def draw_scene(rng):
    trks, cand_lists = T.make_tracklets(int(rng.integers(1 << 30)), LENS, N_CANDS, KINDS)
    c = cand_lists[3]
    cand_lists[3] = [c[0], T.Trk(c[0].boxes.clone(), c[0].ts_list, c[0].score_list, c[0].type), c[2]]     # the tie
    cand_lists[4] = cand_lists[4][::-1]                                 # the best candidate is the last one
    cand_lists[7] = [cand_lists[7][1], cand_lists[7][0], cand_lists[7][2]]       # ... the middle one
    cand_lists[5] = [T.Trk(c.boxes, [x + 50_000 for x in c.ts_list], c.score_list, c.type) for c in cand_lists[5]]   # nothing shared
    return trks, cand_lists


def shared_pairs(trk, cand):
    ci = {ts: i for i, ts in enumerate(cand.ts_list)}
    idx = [(i, ci[ts]) for i, ts in enumerate(trk.ts_list) if ts in ci]
    return np.asarray([i for i, _ in idx], np.int64), np.asarray([j for _, j in idx], np.int64)


def settle(rng, trks, cand_lists, margin):
    for _ in range(300):
        moved = 0
        for trk, cands in zip(trks, cand_lists):
            near = np.zeros(len(trk.ts_list), bool)
            for c in cands:
                i1, i2 = shared_pairs(trk, c)
                if not len(i1):
                    continue
                iou = T.aligned_iou(trk.boxes[i1], c.boxes[i2], torch.float64).numpy()
                yaw = R.canonical_yaw(trk.boxes[i1].numpy(), c.boxes[i2].numpy())
                bad = np.zeros(len(i1), bool)
                for thr in THRESHOLDS:
                    bad |= (np.abs(iou - thr) <= 2 * margin) & (iou > 0)
                for edge in (np.pi / 2, np.pi, 3 * np.pi / 2):
                    bad |= (np.abs(yaw - edge) <= 0.06) & (iou > 0.01)
                near[i1[bad]] = True
            idx = np.nonzero(near)[0]
            moved += len(idx)
            if len(idx):
                trk.boxes[idx, 6] += torch.as_tensor(rng.uniform(0.13, 0.3, len(idx)).astype(np.float32))
                trk.boxes[idx, 0] += torch.as_tensor(rng.uniform(-0.05, 0.05, len(idx)).astype(np.float32))
        if not moved:
            return
    raise RuntimeError('the scene does not settle')


def rigid_pose(rng):
    a = rng.uniform(-np.pi, np.pi)
    m = np.eye(4)
    m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    m[:3, 3] = rng.uniform(-40, 40, 3) * np.array([1, 1, 0.05])
    return m


def host_methods(parts, rng_seed):
    """LiDARTracklet's host methods on one 9-frame tracklet under random rigid poses -> dict of arrays"""
    rng = np.random.default_rng(rng_seed)
    f64 = parts['dtype'] == torch.float64
    dt = parts['dtype']
    n = 9
    boxes = T.track_boxes(rng, n, 0)
    ts = [T.TS0 + 100_000 * i for i in range(n)]
    scores = rng.uniform(0.1, 0.9, n).astype(np.float32)
    poses = np.stack([rigid_pose(rng) for _ in range(n)])
    shared = rigid_pose(rng)
    new_boxes = T.jitter(rng, boxes, 0.5)
    new_scores = rng.uniform(0.1, 0.9, n).astype(np.float32)
    valid = rng.random(n) < 0.7
    valid[0], valid[1] = True, False
    other_ts = ts[2:6] + [ts[-1] + 100_000, ts[-1] + 200_000]
    other = T.jitter(rng, np.concatenate([boxes[2:6], boxes[-2:]]), 0.4)
    out = dict(boxes=boxes, ts=np.asarray(ts, np.int64), scores=scores, poses=poses, shared_pose=shared, new_boxes=new_boxes,
               new_scores=new_scores, valid=valid, other_ts=np.asarray(other_ts, np.int64), other_boxes=other)
    with M.patched(f64):
        def fresh():
            t = ref_tracklet(parts, T.Trk(boxes, ts, scores.tolist(), 0), 'h')
            t.pose_list = [torch.as_tensor(p).to(dt) for p in poses]
            return t
        t = fresh()
        t.frame_transform(torch.as_tensor(shared).to(dt))
        out['frame_transform'] = t.concated_boxes().tensor.numpy()
        out['shared2ego'] = t.shared2ego().tensor.numpy()
        t = fresh()
        t.frame_transform(torch.as_tensor(shared).to(dt))
        t.update_from_prediction(parts['lidar'](torch.as_tensor(new_boxes).to(dt)), torch.as_tensor(new_scores),
                                 torch.zeros(n, dtype=torch.long), torch.as_tensor(valid))
        out['updated_boxes'] = np.concatenate(t.box_list, 0)
        out['updated_scores'] = np.asarray(t.score_list, np.float64)
        for name, call in (('flip_h', lambda t: t.flip('horizontal')), ('flip_v', lambda t: t.flip('vertical')),
                           ('rotate', lambda t: t.rotate(0.37)), ('translate', lambda t: t.translate(torch.tensor([1.5, -2.0, 0.25]).to(dt))),
                           ('scale', lambda t: t.scale(1.1))):
            t = fresh()
            call(t)
            out[name] = t.concated_boxes().tensor.numpy()
        t, o = fresh(), ref_tracklet(parts, T.Trk(other, other_ts, [1.0] * len(other_ts), 0), 'o')
        out['ts_intersection'] = np.asarray(t.ts_intersection(o), np.int64)
        out['self_ious'] = t.self_ious(o).numpy()
        out['intersection_ious'] = t.intersection_ious(o).numpy()
        b, m = o.concated_boxes_from_ts(t.ts_list)
        out['boxes_from_ts'], out['mask_from_ts'] = b.numpy(), m.numpy()
        out['index_from_ts'] = np.asarray([o.get_index_from_ts(x) for x in ts], np.int64)
    return out


def decode_cases(parts, rois, gt_rois, bbox_pred, cls_score, cls_preds, labels_3d, valid):
    f64 = parts['dtype'] == torch.float64
    dt = parts['dtype']
    out = {}
    metas = [dict(box_type_3d=parts['lidar'])] * len(LENS)
    for name, cfg in (('plain', {}), ('identical', dict(identical_decode=True)), ('replace', dict(replace_center=True, replace_size=True,
                                                                                                 replace_yaw=True))):
        head = make_bbox_head(parts, cfg)
        with M.patched(f64):
            res = head.get_bboxes_from_tracklet(torch.as_tensor(rois).to(dt), torch.as_tensor(cls_score).to(dt),
                                                torch.as_tensor(bbox_pred).to(dt), torch.as_tensor(valid), torch.as_tensor(labels_3d),
                                                torch.as_tensor(cls_preds).to(dt), metas, gt_rois=torch.as_tensor(gt_rois).to(dt),
                                                cfg=head.test_cfg)
        boxes, scores = np.concatenate([r[0].tensor.numpy() for r in res]), np.concatenate([r[1].numpy() for r in res])
        if name == 'identical':     # the RoIs and their scores themselves: nothing to store
            assert np.array_equal(boxes, np.asarray(rois)[:, 1:].astype(boxes.dtype)) and np.array_equal(scores, np.asarray(cls_preds).astype(scores.dtype))
            continue
        out[f'decode_{name}_boxes'], out[f'decode_{name}_scores'] = boxes, scores
    return out


def reference_state_keys(name):
    """the state_dict keys of the reference's TrackletDetector for one shipped config: its three parameter-owning modules -
    DynamicScatterVFE, SimpleSparseUNet (oracle.ref_loader.load_reference_spconv) and FullySparseBboxHead (executed from its source
    text; build_loss / build_bbox_coder stood in for by parameter-free objects) - under the attribute names of TrackletDetector,
    TrackletSegmentor and TrackletRoIHead (segmentor.voxel_encoder / segmentor.backbone / roi_head.bbox_head).  TimestampEncoder and
    TrackletPointRoIExtractor own no parameter."""
    from torch import nn
    import torch.nn.functional as F
    from oracle import ref_loader as L
    sp = L.load_reference_spconv()
    ns = sp.base
    runner = sys.modules['mmcv.runner']
    head_cls = L.load_reference_class(M.HEAD_PY, 'FullySparseBboxHead', dict(
        np=np, torch=torch, nn=nn, F=F, BaseModule=runner.BaseModule, force_fp32=runner.force_fp32, auto_fp16=runner.auto_fp16,
        build_loss=lambda cfg: nn.Identity(), build_bbox_coder=lambda cfg: types.SimpleNamespace(code_size=7),
        build_mlp=ns.sst_ops.build_mlp, builder=ns.builder))
    model = eval(open(os.path.join(ROOT, 'tests', 'golden', 'configs', 'ctrl', name + '.model.py')).read())

    def args(cfg):
        cfg = dict(cfg)
        cfg.pop('type')
        return cfg

    vfe = ns.builder.build_voxel_encoder(dict(model['segmentor']['voxel_encoder']))
    unet = sp.sparse_unet.SimpleSparseUNet(**args(model['segmentor']['backbone']))
    head = head_cls(**args(model['roi_head']['bbox_head']))
    return (['segmentor.voxel_encoder.' + k for k in vfe.state_dict()] + ['segmentor.backbone.' + k for k in unet.state_dict()]
            + ['roi_head.bbox_head.' + k for k in head.state_dict()])


def main():
    rng = np.random.default_rng(52317)
    p32, p64 = reference_parts(False), reference_parts(True)
    trks, cand_lists = draw_scene(rng)
    noise_iou = 1e-5
    for attempt in range(6):
        settle(rng, trks, cand_lists, max(1e-4, 10 * noise_iou))
        runs = {(oc, tag): run_targets(parts, trks, cand_lists, bool(oc)) for oc in (0, 1) for tag, parts in (('f32', p32), ('f64', p64))}
        noise_iou = max(float(np.abs(runs[oc, 'f32']['iou'] - runs[oc, 'f64']['iou']).max()) for oc in (0, 1))
        used = runs[0, 'f64']['iou']
        used = used[used > 0]
        if all(np.abs(used - thr).min() > max(1e-4, 10 * noise_iou) for thr in THRESHOLDS):
            break
    else:
        raise RuntimeError('no scene found')
    out = dict(lens=np.asarray(LENS, np.int64), kinds=np.asarray(KINDS, np.int64), n_cands=np.asarray(N_CANDS, np.int64),
               boxes=np.concatenate([t.boxes.numpy() for t in trks]), ts=np.asarray([x for t in trks for x in t.ts_list], np.int64),
               scores=np.asarray([x for t in trks for x in t.score_list], np.float32),
               cand_lens=np.asarray([len(c.ts_list) for cs in cand_lists for c in cs], np.int64),
               cand_boxes=np.concatenate([c.boxes.numpy() for cs in cand_lists for c in cs]),
               cand_ts=np.asarray([x for cs in cand_lists for c in cs for x in c.ts_list], np.int64), noise_iou=np.float64(noise_iou))
    rel = lambda a, b: float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-30))   # noqa: E731
    for oc in (0, 1):
        r32, r64 = runs[oc, 'f32'], runs[oc, 'f64']
        for k in ('chosen', 'assigned_gt_inds', 'frame_inds', 'counts', 'reg_mask', 'labels', 'roi_frame_inds', 'labels_3d'):
            assert np.array_equal(r32[k], r64[k]), k
            if oc or k not in ('roi_frame_inds', 'labels_3d'):
                out[f'oc{oc}_{k}'] = r32[k].astype(np.int32 if k in ('frame_inds', 'assigned_gt_inds', 'labels', 'roi_frame_inds', 'labels_3d') else r32[k].dtype)
        # the RoIs of the tracklets do not depend on the assigner: stored once (object_centric on)
        for k in ('iou', 'soft_label', 'targets') + (('gt_rois', 'rois', 'cls_preds') if oc else ()):
            out[f'oc{oc}_{k}_f64'] = r64[k].astype(np.float64)
            out[f'noise_oc{oc}_{k}'] = np.float64(rel(r32[k], r64[k]) if r64[k].size and np.abs(r64[k]).max() else 0.0)
        print('object_centric', oc, 'chosen', r64['chosen'].tolist(), 'counts', r64['counts'].tolist(),
              {k: float(out[f'noise_oc{oc}_{k}']) for k in ('iou', 'soft_label', 'targets')})
    assert out['oc0_chosen'][3] == 0 and out['oc0_chosen'][4] == 2 and out['oc0_chosen'][7] == 1 and out['oc0_counts'][5][0] == 0 and out['oc0_counts'][1][0] == 0 and out['oc0_chosen'][1] == -1
    # decoding: predictions exactly representable in float16
    n = int(sum(LENS))
    bbox_pred = M.f16(rng.normal(0, 1, (n, 7)) * np.array([0.3, 0.3, 0.3, 0.2, 0.2, 0.2, 0.4]))
    cls_score = M.f16(rng.normal(0, 2, (n, 1)))
    valid = rng.random(n) < 0.85
    r64 = runs[1, 'f64']
    out.update(bbox_pred=bbox_pred.astype(np.float16), cls_score=cls_score.astype(np.float16), roi_valid=valid)
    d32 = decode_cases(p32, r64['rois'], r64['gt_rois'], bbox_pred, cls_score, r64['cls_preds'], r64['labels_3d'], valid)
    d64 = decode_cases(p64, r64['rois'], r64['gt_rois'], bbox_pred, cls_score, r64['cls_preds'], r64['labels_3d'], valid)
    for k in d64:
        out[k + '_f64'] = d64[k].astype(np.float64)
        out['noise_' + k] = np.float64(rel(d32[k], d64[k]))
    h32, h64 = host_methods(p32, 991), host_methods(p64, 991)
    for k in h64:
        if h64[k].dtype.kind == 'f' and k not in ('boxes', 'scores', 'new_boxes', 'new_scores', 'other_boxes', 'poses', 'shared_pose'):
            out['host_' + k + '_f64'] = h64[k].astype(np.float64)
            out['noise_host_' + k] = np.float64(rel(np.asarray(h32[k], np.float64), h64[k]) if h64[k].size else 0.0)
        else:
            out['host_' + k] = h64[k]
    for name in ('ctrl_veh_24e', 'ctrl_ped_24e', 'ctrl_cyc_12e'):
        out['state_keys_' + name] = np.asarray(reference_state_keys(name))
    path = os.path.join(ROOT, 'tests', 'golden', 'tracklet_train.npz')
    np.savez_compressed(path, **out)
    print('noise_iou', noise_iou, {k: float(v) for k, v in out.items() if k.startswith('noise_host') or k.startswith('noise_decode')})
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
