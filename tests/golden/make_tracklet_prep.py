"""Generates tests/golden/tracklet_prep.npz: the tracklet affinities, candidate lists and statistics, the per-box point crops and
the keep masks of CTRL's offline stage as the REFERENCE computes them (data only).

Needs the reference tree (oracle.ref_loader) and oracle/_ref/points_in_boxes_ref.so; run from the repository root:
    python tests/golden/make_tracklet_prep.py

Executed from their source text: LiDARTracklet.max_iou / ts_iou / ts_intersection (core/bbox/structures/lidar_tracklet.py),
LiDARInstance3DBoxes.enlarged_box / enlarged_box_hw / points_in_boxes and its constructor's origin shift (lidar_box3d.py,
base_box3d.py), tracklet_assign and stats (tools/ctrl/generate_candidates.py), extract_and_save_point
(tools/ctrl/generate_track_input.py), process_single_frame and get_grouping_mask (tools/ctrl/remove_empty.py) - the classes loaded
as tests/golden/make_tracklet.py loads them.  Stand-ins for what those texts import from packages that are not in the reference's
tree, or run on CUDA only:
  Tensor.cuda(), torch.cuda.set_device   the identity / nothing (make_roi_head_train.patched)
  TorchEx boxes_overlap_1to1             the stand-in of make_tracklet.py (tests/box_ops_ref.py)
  points_in_boxes_gpu                    float32: the reference's compiled points_in_boxes_cpu (oracle/_ref), the smallest index of
                                         a box that holds the point; float64: the same test in numpy float64
  get_pc_from_time_stamp                 the scene's points of that timestamp
  np.save, print                         recorders (the crops a tracklet collected before free_pc; the two rates ``stats`` prints)
Every case runs in float32 and in float64; noise_aff is the largest gap between the two affinity runs.  The thresholds come from the
reference's tools/ctrl/data_configs/fsd_base_vehicle.yaml (tests/golden/configs/ctrl_data): affinity_thresh 0.5, extra_width 1.
The scene is re-drawn until, in float64, no pair's affinity lies within max(1e-4, 10 noise_aff) of affinity_thresh, and no point
lies within 1e-4 of a face of a box it is tested against; the script asserts both.

The affinity scene: 2 segments, the second without ground truth; 6 predicted tracklets of lengths 1, 63, 64, 65, 200 and 12, 5
ground-truth tracklets; pairs share 0, 1, 64 and 65 timestamps; ground truth 3 has timestamps outside every predicted tracklet;
ground truths 1 and 2 are the same boxes (they tie on predicted tracklet 2); ground truth 4's box at predicted tracklet 0's only
frame touches that box at a corner only.  The crop scene: 3 tracklets over 11 frames (one frame without a box, two tracklets whose
enlarged boxes overlap), 6 point columns.  The remove-empty scene: 4 frames, one without a point in any box, one without a box.
"""
import contextlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'tests'), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import tracklet_ref as T  # noqa: E402
import tracklet_prep_ref as P  # noqa: E402
import make_roi_head_train as M  # noqa: E402
import make_tracklet as MT  # noqa: E402

CAND_PY = 'tools/ctrl/generate_candidates.py'
INPUT_PY = 'tools/ctrl/generate_track_input.py'
EMPTY_PY = 'tools/ctrl/remove_empty.py'
PD_LENS = [1, 63, 64, 65, 200, 12]
REMOVE_EMPTY = {'vehicle': {'bottom_lift': 0.2, 'extra_hw': 0.0, 'box_grouping': True, 'group_size': 1},       # remove_empty.py:155-160
                'pedestrian': {'bottom_lift': 0.1, 'extra_hw': 0.0, 'box_grouping': True, 'group_size': 1},
                'cyclist': {'bottom_lift': 0.1, 'extra_hw': 0.0, 'box_grouping': True, 'group_size': 1}}


class TorchProxy(object):
    """``torch`` as the tool scripts see it: set_device does nothing (and, in the float64 run, float32 reads as float64)"""

    def __init__(self, tm):
        self._tm = tm
        self.cuda = types.SimpleNamespace(set_device=lambda *a, **k: None)

    def __getattr__(self, name):
        return getattr(self._tm, name)


def reference_parts(f64):
    from oracle import build_ref
    parts = MT.reference_parts(f64)
    pib = build_ref.load_points_in_boxes()
    assert pib is not None, 'oracle/_ref/points_in_boxes_ref.so is missing: run build() first'

    def points_in_boxes_gpu(points, boxes):
        pts, bx = points[0], boxes[0]
        if f64:
            m = P.membership_f64(bx.numpy(), pts.numpy())
        else:
            flags = torch.zeros((bx.size(0), pts.size(0)), dtype=torch.int32)
            pib.points_in_boxes_cpu(bx.float().contiguous(), pts.float().contiguous(), flags)
            m = flags.numpy() != 0
        first = np.where(m.any(0), m.argmax(0), -1) if m.shape[0] else np.full(m.shape[1], -1)
        return torch.as_tensor(first.astype(np.int32))[None]

    parts['lidar'].points_in_boxes.__globals__['points_in_boxes_gpu'] = points_in_boxes_gpu
    parts['tm'] = TorchProxy(MT.TorchAsFloat64() if f64 else torch)
    parts['npdt'] = np.float64 if f64 else np.float32
    return parts


def ref_tracklet(parts, trk):
    boxes = trk.boxes.numpy().astype(np.float32)
    t = parts['tracklet'](trk.segment_name, trk.id, int(trk.type), trk.in_world, [boxes[i:i + 1] for i in range(len(boxes))],
                          list(trk.ts_list), [float(s) for s in trk.score_list])
    t.freeze()
    return t


# ---- the affinity scene -------------------------------------------------------------------------------------------------------------

def draw_affinity_scene(rng):
    seg = ['segA'] * 5 + ['segB']
    frames = [[10], range(0, 63), range(0, 64), range(0, 65), range(20, 220), range(0, 12)]
    kinds = [0, 0, 1, 2, 0, 1]
    paths, pd = [], []
    for k, fr in enumerate(frames):
        fr = list(fr)
        path = T.track_boxes(rng, 230, kinds[k])
        paths.append(path)
        pred = T.jitter(rng, path[fr], rng.choice([0.3, 1.0], len(fr))[:, None])
        pd.append(P.Trk(pred, P.frames_ts(fr), rng.uniform(0.1, 0.95, len(fr)).astype(np.float32).tolist(), [1, 1, 2, 4, 1, 2][k],
                        seg[k], f'pd{k}'))
    # pd0: one axis-aligned box; gt4's box of that frame touches it at a corner only
    pd[0].boxes[0, 6] = 0.0
    b0 = pd[0].boxes[0].numpy()
    corner = b0.copy()
    corner[3:6] = (1.5, 3.25, 1.5)
    corner[0] = b0[0] + (b0[3] + corner[3]) / 2
    corner[1] = b0[1] + (b0[4] + corner[4]) / 2
    corner[2] = b0[2]
    gt = []

    def make(k, fr, path, boxes=None, kind=1):
        fr = list(fr)
        gt.append(P.Trk(path[fr] if boxes is None else boxes, P.frames_ts(fr), [1.0] * len(fr), kind, 'segA', f'gt{k}'))

    make(0, range(0, 65), paths[3], kind=4)                                    # 65 shared with pd3, 64 with pd2, 1 with pd0
    make(1, range(0, 70), paths[2], kind=2)                                    # 64 shared with pd2
    make(2, range(0, 70), paths[2], kind=2)                                    # the same boxes: a tie on pd2
    gt.append(P.Trk(paths[1][:30], [x + 50_000 for x in P.frames_ts(range(0, 30))], [1.0] * 30, 1, 'segA', 'gt3'))   # outside every pd
    fr4 = [10] + list(range(70, 160))
    make(4, fr4, paths[4], np.concatenate([corner[None], paths[4][fr4[1:]]], 0).astype(np.float32))   # 1 shared with pd0 .. pd3
    return pd, gt


def shared_counts(pd, gt):
    return np.asarray([[len(set(a.ts_list) & set(b.ts_list)) for b in gt] for a in pd], np.int64)


def run_affinity(parts, pd, gt, thresh):
    L = __import__('oracle.ref_loader', fromlist=['x'])
    f64 = parts['dtype'] == torch.float64
    glb = dict(torch=parts['tm'])
    assign = L.load_reference_function(CAND_PY, 'tracklet_assign', dict(glb, print=lambda *a, **k: None))
    said = []
    stats = L.load_reference_function(CAND_PY, 'stats', dict(glb, print=lambda s: said.append(s)))
    list2dict = L.load_reference_function(CAND_PY, 'tracklet_list2dict', dict(defaultdict=__import__('collections').defaultdict))
    with M.patched(f64):
        rp, rg = [ref_tracklet(parts, t) for t in pd], [ref_tracklet(parts, t) for t in gt]
        aff = np.asarray([[a.max_iou(b) for b in rg] if a.segment_name == 'segA' else [] for a in rp][:5], np.float64)
        ts_iou = np.asarray([[a.ts_iou(b) for b in rg] for a in rp], np.float64)
        inter = np.asarray([[len(a.ts_intersection(b)) for b in rg] for a in rp], np.int64)
        for t in rp + rg:
            t.to_collate_format()
        pd_dict, gt_dict = list2dict(rp), list2dict(rg)
        out, counter = {}, []
        assign(pd_dict, gt_dict, list(pd_dict.keys()), out, counter, dict(candidate=dict(affinity_thresh=thresh)))
        assert len(counter) == len(pd_dict) and all(t.uuid in out for t in rp if t.segment_name == 'segA'), 'tracklet_assign failed'
        to_save = [out.get(t.uuid, []) for t in rp]                        # list_to_save, generate_candidates.py:130
        cands = [[int(c[1][2:]) for c in cl] for cl in to_save]            # the id 'gt<k>' of every dumped candidate
        stats(rp, to_save)
    rates = [float(s.split(':')[1]) for s in said]
    return dict(aff=aff, ts_iou=ts_iou, inter=inter, cands=cands, stats=np.asarray(rates, np.float64))


# ---- the crop scene -----------------------------------------------------------------------------------------------------------------

def draw_crop_scene(rng, extra_width):
    path = T.track_boxes(rng, 12, 0)
    other = T.track_boxes(rng, 12, 1)
    near = path.copy()
    near[:, 0] += 1.0                      # within reach of the enlarged boxes of ``path``: points in several boxes
    near[:, 3:6] *= 0.8
    sets = [(list(range(0, 5)), path), (list(range(2, 10)), other), ([1, 3, 4, 9], near)]
    trks = [P.Trk(b[fr], P.frames_ts(fr), [0.5] * len(fr), 1, 'segA', f'c{k}') for k, (fr, b) in enumerate(sets)]
    frames = {}
    for f in range(11):                    # frame 10 holds no box
        ts = P.frames_ts([f])[0]
        boxes = [t.boxes[t.ts_list.index(ts)].numpy() for t in trks if ts in t.ts_list]
        enl = P.enlarged_box(np.stack(boxes), extra_width) if boxes else np.zeros((0, 7), np.float32)
        frames[ts] = P.points_around(rng, enl, 160 if boxes else 0, 140, 6)
        if len(enl):
            assert P.face_clearance(enl, frames[ts]).min() >= 1e-4
    return trks, frames


def run_crops(parts, trks, frames, extra_width):
    L = __import__('oracle.ref_loader', fromlist=['x'])
    f64 = parts['dtype'] == torch.float64
    saved = []
    fake_np = types.SimpleNamespace(save=lambda fw, pc: saved.append([np.asarray(p) for p in pc]))
    fn = L.load_reference_function(INPUT_PY, 'extract_and_save_point', dict(
        torch=parts['tm'], np=fake_np, osp=os.path, print=lambda *a, **k: None,
        get_pc_from_time_stamp=lambda ts, ts2idx, root, split: frames[ts].astype(parts['npdt'])))
    with M.patched(f64), tempfile.TemporaryDirectory() as tmp:
        rt = [ref_tracklet(parts, t) for t in trks]
        for t in rt:
            t.to_collate_format()
        num_pts, counter = {}, []
        fn(dict(split='val', box=dict(extra_width=extra_width)), {'segA': rt}, num_pts, ['segA'], {'segA': sorted(frames)}, None, None, tmp,
           counter)
    assert counter == [0] and len(saved) == len(trks), 'extract_and_save_point failed'
    assert num_pts['segA'] == [[len(p) for p in pcs] for pcs in saved]
    return saved, num_pts['segA']


# ---- the remove-empty scene -----------------------------------------------------------------------------------------------------------

def modified(boxes, lift):
    """the boxes process_single_frame tests: bottom-centred, lifted, enlarged_box_hw(0.0)"""
    m = P.to_bottom_centre(np.asarray(boxes, np.float32).reshape(-1, 7), (0.5, 0.5, 0.5))
    m[:, 2] += m[:, 5] * np.float32(lift)
    return P.enlarged_box_hw(m, 0.0)


def draw_empty_scene(rng):
    boxes_list, points_list = [], []
    for f, nb in enumerate([6, 4, 0, 5]):
        b = np.concatenate([T.track_boxes(rng, 1, k % 3) for k in range(nb)] + [np.zeros((0, 7), np.float32)], 0)
        b[:, 2] += b[:, 5] * np.float32(0.5)          # gravity-centred, as bin2lidarboxes hands them on
        boxes_list.append(b.astype(np.float32))
        tested = [modified(b, lift) for lift in (0.1, 0.2)]
        n_hit = max(nb - 2, 0) if f != 1 else 0               # frame 1: no box holds a point; elsewhere the last two boxes are empty
        pts = P.points_around(rng, tested[1][:n_hit], 20 * n_hit, 60, 3)
        far = np.ones(len(pts), bool)
        for t in tested:
            if len(t):
                far &= ~P.membership(t[n_hit:], pts).any(0)         # nothing in the boxes meant to be empty
        pts = pts[far]
        for t in tested:
            if len(t):
                assert P.face_clearance(t, pts).min() >= 1e-4
        points_list.append(np.ascontiguousarray(pts))
    return boxes_list, points_list


def run_empty(parts, boxes_list, points_list, config):
    L = __import__('oracle.ref_loader', fromlist=['x'])
    f64 = parts['dtype'] == torch.float64
    glb = dict(torch=parts['tm'], print=lambda *a, **k: None)
    grouping = L.load_reference_function(EMPTY_PY, 'get_grouping_mask', dict(glb))
    fn = L.load_reference_function(EMPTY_PY, 'process_single_frame', dict(
        glb, get_grouping_mask=grouping, get_pc_from_time_stamp=lambda ts, ts2idx, root, split: points_list[ts - P.TS0].astype(parts['npdt'])))
    saved = {k: sys.modules.get(k) for k in ('mmdet3d', 'mmdet3d.core')}
    pkg = types.ModuleType('mmdet3d')
    pkg.__path__ = []
    core = types.ModuleType('mmdet3d.core')
    core.LiDARInstance3DBoxes = parts['lidar']
    sys.modules['mmdet3d'], sys.modules['mmdet3d.core'] = pkg, core
    try:
        with M.patched(f64):
            input_list = [(np.arange(len(b)), b.astype(parts['npdt']), np.arange(len(b)), 'segA', P.TS0 + f) for f, b in enumerate(boxes_list)
                          if len(b)]           # bin2lidarboxes yields no frame without an object
            out = []
            fn(config, None, out, input_list, None, 'training', 0, 1)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    assert len(out) == len(input_list), 'process_single_frame failed'
    masks = [np.zeros(len(b), bool) for b in boxes_list]
    for valid_box, valid_ids, _, ts in out:
        masks[ts - P.TS0][np.asarray(valid_ids, np.int64)] = True
    return masks


def box_methods(parts):
    """enlarged_box / enlarged_box_hw with a positive and a negative width (the negative one restores boxes it would invert)"""
    f64 = parts['dtype'] == torch.float64
    boxes = np.array([[1, 2, -1, 2.0, 4.5, 1.7, 0.3], [5, -3, 0, 0.5, 0.9, 1.75, -1.2], [0, 0, 0, 0.8, 0.3, 0.25, 2.0]], np.float32)
    with M.patched(f64):
        b = parts['lidar'](torch.as_tensor(boxes.astype(parts['npdt'])))
        out = {f'enl_{tag}': getattr(b, name)(w).tensor.numpy() for name, tag, w in (
            ('enlarged_box', 'pos', 1), ('enlarged_box', 'neg', -0.2), ('enlarged_box_hw', 'hw_pos', 0.25), ('enlarged_box_hw', 'hw_neg', -0.2))}
        out['enl_origin'] = parts['lidar'](torch.as_tensor(boxes.astype(parts['npdt'])), origin=(0.5, 0.5, 0.5)).tensor.numpy()
    out['enl_in'] = boxes
    return out


def main():
    cfg = P.data_config('fsd_base_vehicle')
    thresh, extra_width = cfg['candidate']['affinity_thresh'], cfg['box']['extra_width']
    assert thresh == 0.5 and extra_width == 1
    p32, p64 = reference_parts(False), reference_parts(True)
    rng = np.random.default_rng(90417)
    for attempt in range(50):
        pd, gt = draw_affinity_scene(rng)
        a32, a64 = run_affinity(p32, pd, gt, thresh), run_affinity(p64, pd, gt, thresh)
        noise = float(np.abs(a32['aff'] - a64['aff']).max())
        margin = max(1e-4, 10 * noise)
        if np.abs(a64['aff'] - thresh).min() > margin and a32['cands'] == a64['cands'] and max(a64['aff'][2, 1], a64['aff'][3, 0]) > thresh:
            break
    else:
        raise RuntimeError('no affinity scene found')
    assert np.abs(a64['aff'] - thresh).min() > max(1e-4, 10 * noise)
    inter = shared_counts(pd, gt)
    assert np.array_equal(inter, a64['inter']) and np.array_equal(a32['ts_iou'], a64['ts_iou']) and np.array_equal(a32['stats'], a64['stats'])
    assert {0, 1, 64, 65} <= set(inter[:5].reshape(-1).tolist()) and (inter[:, 3] == 0).all()
    assert a64['aff'][2, 1] == a64['aff'][2, 2] and a32['aff'][2, 1] == a32['aff'][2, 2] and a64['cands'][5] == [] and inter[0, 4] == 1
    print('affinity (float64):\n', np.round(a64['aff'], 4), '\nshared:\n', inter, '\ncandidates', a64['cands'], 'stats', a64['stats'],
          'noise', noise, 'corner pair', a32['aff'][0, 4], a64['aff'][0, 4])

    out = dict(thresh=np.float64(thresh), extra_width=np.float64(extra_width), noise_aff=np.float64(noise), aff_f64=a64['aff'],
               ts_iou=a64['ts_iou'], shared=inter, cand_counts=np.asarray([len(c) for c in a64['cands']], np.int64),
               cand_flat=np.asarray([g for c in a64['cands'] for g in c], np.int64), stats=a64['stats'])
    for tag, trks in (('pd', pd), ('gt', gt)):
        out[f'{tag}_lens'] = np.asarray([len(t) for t in trks], np.int64)
        out[f'{tag}_boxes'] = np.concatenate([t.boxes.numpy() for t in trks]).astype(np.float32)
        out[f'{tag}_ts'] = np.asarray([x for t in trks for x in t.ts_list], np.int64)
        out[f'{tag}_scores'] = np.asarray([x for t in trks for x in t.score_list], np.float32)
        out[f'{tag}_types'] = np.asarray([t.type for t in trks], np.int64)
        out[f'{tag}_segs'] = np.asarray([t.segment_name for t in trks])

    trks, frames = draw_crop_scene(rng, extra_width)
    c32, n32 = run_crops(p32, trks, frames, extra_width)
    c64, n64 = run_crops(p64, trks, frames, extra_width)
    assert n32 == n64 and all(np.array_equal(a, b.astype(np.float32)) for x, y in zip(c32, c64) for a, b in zip(x, y))
    flat = [p for pcs in c32 for p in pcs]
    assert sum(len(p) for p in flat) > 200 and any(len(p) == 0 for p in flat) is not None
    out.update(crop_lens=np.asarray([len(t) for t in trks], np.int64), crop_boxes=np.concatenate([t.boxes.numpy() for t in trks]),
               crop_ts=np.asarray([x for t in trks for x in t.ts_list], np.int64), crop_frame_ts=np.asarray(sorted(frames), np.int64),
               crop_frame_lens=np.asarray([len(frames[ts]) for ts in sorted(frames)], np.int64),
               crop_points=np.concatenate([frames[ts] for ts in sorted(frames)]).astype(np.float32),
               crop_num_pts=np.asarray([n for ns in n32 for n in ns], np.int64), crop_rows=np.concatenate(flat).astype(np.float32))
    print('crops: points per (tracklet, frame)', n32)

    boxes_list, points_list = draw_empty_scene(rng)
    out.update(re_box_lens=np.asarray([len(b) for b in boxes_list], np.int64), re_boxes=np.concatenate(boxes_list).astype(np.float32),
               re_pt_lens=np.asarray([len(p) for p in points_list], np.int64), re_points=np.concatenate(points_list).astype(np.float32))
    for name, config in REMOVE_EMPTY.items():
        m32, m64 = run_empty(p32, boxes_list, points_list, config), run_empty(p64, boxes_list, points_list, config)
        assert all(np.array_equal(a, b) for a, b in zip(m32, m64))
        out[f're_mask_{name}'] = np.concatenate(m32)
        out[f're_lift_{name}'], out[f're_hw_{name}'] = np.float64(config['bottom_lift']), np.float64(config['extra_hw'])
        print('remove_empty', name, [m.astype(int).tolist() for m in m32])
    assert not out['re_mask_vehicle'][6:10].any() and out['re_mask_vehicle'][:4].all() and not out['re_mask_vehicle'][4:6].any()

    b32, b64 = box_methods(p32), box_methods(p64)
    for k in b64:
        out[k] = b32[k].astype(np.float32)
        assert np.abs(b32[k] - b64[k]).max() < 1e-6
    path = os.path.join(HERE, 'tracklet_prep.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
