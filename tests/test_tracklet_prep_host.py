"""CTRL's offline stage without a GPU: the CPU restatement (tests/tracklet_prep_ref.py) against the reference's own results
(tests/golden/tracklet_prep.npz), the host methods the stage adds to sst_amd.LiDARTracklet against the same file, the refusals, and
the header / binding consistency of the new entry points.  Candidate lists, crops, counts, keep masks and the two statistics match
exactly; the float32 affinity within max(4 x the reference's own float32-vs-float64 gap, 1e-6), the float64 one within that gap."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

import tracklet_ref as T
import tracklet_prep_ref as P


@pytest.fixture(scope='module')
def gold():
    return load_golden('tracklet_prep.npz')


def gold_candidates(g):
    return [c.tolist() for c in P.split(g['cand_flat'], g['cand_counts'])]


def test_thresholds_come_from_the_reference_data_configs(gold):
    cfg = P.data_config('fsd_base_vehicle')        # the golden's: the vehicle configuration
    assert cfg['candidate']['affinity_thresh'] == float(gold['thresh']) == 0.5 and cfg['box']['extra_width'] == float(gold['extra_width']) == 1
    for name, thresh, width in (('fsd_base_pedestrian', 0.2, 1), ('fsd_base_cyc', 0.2, 2)):
        cfg = P.data_config(name)
        assert cfg['candidate']['affinity_thresh'] == thresh and cfg['box']['extra_width'] == width


def test_scene_has_the_cases_the_kernel_can_get_wrong(gold):
    pd, gt = P.gold_scene(gold)
    assert [len(t) for t in pd] == [1, 63, 64, 65, 200, 12] and len(gt) == 5
    assert {t.segment_name for t in gt} == {'segA'} and pd[5].segment_name == 'segB'
    shared = gold['shared']
    assert {0, 1, 64, 65} <= set(shared[:5].reshape(-1).tolist()) and (shared[:, 3] == 0).all() and shared[0, 4] == 1
    assert np.array_equal(pd_gt(gt, 1).boxes, pd_gt(gt, 2).boxes)                 # the tie
    assert gold['aff_f64'][2, 1] == gold['aff_f64'][2, 2] > 0.5 and gold['aff_f64'][0, 4] == 0.0    # ... and the corner pair
    margin = max(1e-4, 10 * float(gold['noise_aff']))
    assert np.abs(gold['aff_f64'] - 0.5).min() > margin


def pd_gt(trks, k):
    return trks[k]


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_restated_affinity_candidates_and_statistics_equal_the_reference(gold, dtype):
    pd, gt = P.gold_scene(gold)
    aff = P.affinity(pd, gt, dtype)
    assert [a[0].tolist() for a in aff] == [list(range(5))] * 5 + [[]]
    got = np.stack([a[1] for a in aff[:5]]).astype(np.float64)
    gap = float(gold['noise_aff'])
    err = float(np.abs(got - gold['aff_f64']).max())
    limit = max(gap, 1e-12) if dtype == torch.float64 else T.bar(gap)
    print(dtype, 'err', err, 'gap', gap)
    assert err <= limit
    cands = P.candidates(aff, float(gold['thresh']))
    assert cands == gold_candidates(gold) and cands[5] == [] and cands[2] == [1, 2]
    assert P.stats([len(t) for t in pd], cands) == tuple(gold['stats'].tolist())


def test_restated_crops_and_counts_equal_the_reference(gold):
    trks, frames = P.gold_crop_scene(gold)
    pcs = P.crop_tracklets(trks, frames, float(gold['extra_width']))
    flat = [p for tr in pcs for p in tr]
    assert [len(p) for p in flat] == gold['crop_num_pts'].tolist() and [len(tr) for tr in pcs] == gold['crop_lens'].tolist()
    assert np.array_equal(np.concatenate(flat), gold['crop_rows'])
    # the same through the batch form: (frame, box, ascending point index)
    ts_sorted = sorted(frames)
    boxes_list = [P.enlarged_box(np.stack([t.boxes[t.ts_list.index(ts)].numpy() for t in trks if ts in t.ts_list] + [np.zeros(7, np.float32)])[:-1], 1)
                  for ts in ts_sorted]
    rows, src, counts = P.crops([frames[ts] for ts in ts_sorted], boxes_list)
    assert counts.sum() == len(rows) == len(gold['crop_rows']) and sorted(counts.tolist()) == sorted(gold['crop_num_pts'].tolist())
    k = 0
    for f, ts in enumerate(ts_sorted):
        for _ in range(len(boxes_list[f])):
            n = counts[k]
            o = counts[:k].sum()
            assert np.array_equal(rows[o:o + n], frames[ts][src[o:o + n]]) and (np.diff(src[o:o + n]) > 0).all()
            k += 1
    assert (P.membership(boxes_list[1], frames[ts_sorted[1]]).sum(0) >= 2).any()       # a point inside several boxes


def test_restated_keep_masks_equal_the_reference(gold):
    boxes_list, points_list = P.split(gold['re_boxes'], gold['re_box_lens']), P.split(gold['re_points'], gold['re_pt_lens'])
    for name in ('vehicle', 'pedestrian', 'cyclist'):
        masks, dropped = P.keep_masks(boxes_list, points_list, float(gold[f're_lift_{name}']), float(gold[f're_hw_{name}']))
        assert np.array_equal(np.concatenate(masks), gold[f're_mask_{name}'])
        assert dropped == [False, True, True, False]


def test_box_modifications_equal_the_reference(gold):
    from sst_amd import tracklet_prep as TP
    boxes = gold['enl_in']
    t = torch.as_tensor(boxes)
    for tag, fn, ref, w in (('pos', TP.enlarged_box, P.enlarged_box, 1), ('neg', TP.enlarged_box, P.enlarged_box, -0.2),
                            ('hw_pos', TP.enlarged_box_hw, P.enlarged_box_hw, 0.25), ('hw_neg', TP.enlarged_box_hw, P.enlarged_box_hw, -0.2)):
        assert np.array_equal(fn(t, w).numpy(), gold[f'enl_{tag}']), tag
        assert np.array_equal(ref(boxes, w), gold[f'enl_{tag}']), tag
    assert np.array_equal(gold['enl_neg'][2], boxes[2]) and not np.array_equal(gold['enl_neg'][0], boxes[0])     # restored / shrunk
    assert np.array_equal(P.to_bottom_centre(boxes, (0.5, 0.5, 0.5)), gold['enl_origin'])
    assert torch.equal(t, torch.as_tensor(boxes))                                                               # inputs untouched


def test_timestamp_methods_and_point_lists_of_the_tracklet(gold):
    pd, gt = P.gold_scene(gold)
    lp, lg = [P.lidar(t) for t in pd], [P.lidar(t) for t in gt]
    got = np.asarray([[a.ts_iou(b) for b in lg] for a in lp])
    assert np.array_equal(got, gold['ts_iou'])
    assert np.array_equal(np.asarray([[len(a.ts_intersection(b)) for b in lg] for a in lp]), gold['shared'])
    t = lp[5]
    t.append_pc(np.zeros((3, 6), np.float32), t.ts_list[0])
    t.append_pc(np.zeros((0, 6), np.float32))
    with pytest.raises(AssertionError):
        t.append_pc(np.zeros((1, 6), np.float32), t.ts_list[5])           # not the next frame
    assert [len(p) for p in t.pc_list] == [3, 0]
    t.free_pc()
    assert t.pc_list is None


def test_candidate_statistics_of_the_library_equal_the_reference(gold):
    import sst_amd
    pd, gt = P.gold_scene(gold)
    cands = [[gt[g] for g in c] for c in gold_candidates(gold)]
    assert sst_amd.candidate_stats(pd, cands) == tuple(gold['stats'].tolist())
    assert sst_amd.tracklet_prep.REMOVE_EMPTY_DEFAULTS['vehicle']['bottom_lift'] == float(gold['re_lift_vehicle'])
    assert sst_amd.tracklet_prep.REMOVE_EMPTY_DEFAULTS['cyclist']['bottom_lift'] == float(gold['re_lift_cyclist'])


@pytest.mark.parametrize('struct,cname', [('TrackletAffinityArgs', 'sst_tracklet_affinity_args'), ('BoxCropsArgs', 'sst_box_crops_args')])
def test_argument_structs_match_the_header(struct, cname):
    """field names and order of the ctypes structures == the typedefs of include/sst_amd.h"""
    from sst_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'sst_amd.h')).read()
    body = re.search(r'typedef struct ' + cname + r' \{(.*?)\} ' + cname + ';', text, re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = re.sub(r'^(const\s+)?(int64_t|int32_t|uint8_t|float|double|void)\b', '', decl.strip())
        fields += [re.sub(r'[\s\*]|\[.*?\]', '', f) for f in decl.split(',') if f.strip()]
    assert fields == [f[0] for f in getattr(_lib, struct)._fields_]


def test_library_answers_the_launch_constants_without_a_gpu():
    from sst_amd import _lib
    lib = _lib.load()
    assert lib.sst_tracklet_affinity_pairs_per_block() == 4
    assert lib.sst_box_crops_tile() == 4096 and lib.sst_box_crops_box_chunk() == 128
    assert lib.sst_box_crops_workspace_bytes(1000) >= lib.sst_scan_workspace_bytes(1000)
    assert lib.sst_tracklet_affinity_f32(None, None) == _lib.SST_ERR_ARG
    assert lib.sst_box_crops_count_f32(None, None) == _lib.SST_ERR_ARG and lib.sst_box_crops_fill_f32(None, None) == _lib.SST_ERR_ARG
    import ctypes
    a = _lib.BoxCropsArgs()
    a.cols = 2
    assert lib.sst_box_crops_count_f32(ctypes.byref(a), None) == _lib.SST_ERR_ARG            # C < 3
    b = _lib.TrackletAffinityArgs()
    b.n_pd = -1
    assert lib.sst_tracklet_affinity_f32(ctypes.byref(b), None) == _lib.SST_ERR_ARG


def test_refusals_by_name():
    import sst_amd
    pts, boxes = torch.zeros(5, 4), torch.zeros(2, 7)
    for fn in (sst_amd.box_point_crops, sst_amd.box_point_counts):
        with pytest.raises(RuntimeError, match='box widths other than 7'):
            fn([pts], [torch.zeros(2, 9)])
        with pytest.raises(RuntimeError, match='float32'):
            fn([pts.double()], [boxes])
        with pytest.raises(RuntimeError, match='float32'):
            fn([pts], [boxes.half()])
        with pytest.raises(RuntimeError, match='C >= 3'):
            fn([torch.zeros(5, 2)], [boxes])
        with pytest.raises(RuntimeError, match='one box tensor per frame'):
            fn([pts, pts], [boxes])
    with pytest.raises(NotImplementedError, match='group_size=2'):
        sst_amd.remove_empty_boxes([boxes], [pts], 0.2, 0.0, box_grouping=True, group_size=2)
    with pytest.raises(NotImplementedError, match='box_grouping=False'):
        sst_amd.remove_empty_boxes([boxes], [pts], 0.2, 0.0, box_grouping=False)
    with pytest.raises(RuntimeError, match='box widths other than 7'):
        sst_amd.remove_empty_boxes([torch.zeros(2, 9)], [pts], 0.2)

    def trk(width=7, dtype=torch.float32, seg='s'):
        t = sst_amd.LiDARTracklet(seg, 'a', 1, True, torch.zeros(2, width), [T.TS0, T.TS0 + 100_000], [0.5, 0.5])
        t.freeze()
        t.boxes = t.boxes.to(dtype)
        return t

    with pytest.raises(RuntimeError, match='box widths other than 7'):
        sst_amd.tracklet_affinity([trk(9)], [trk()])
    with pytest.raises(RuntimeError, match='float32'):
        sst_amd.tracklet_affinity([trk()], [trk(dtype=torch.float64)])
    with pytest.raises(RuntimeError, match='box widths other than 7'):
        sst_amd.crop_tracklet_points([trk(9)], {T.TS0: np.zeros((4, 3), np.float32)}, 1)
    with pytest.raises(RuntimeError, match='C >= 3'):
        sst_amd.crop_tracklet_points([trk()], {T.TS0: np.zeros((4, 2), np.float32)}, 1)
    with pytest.raises(RuntimeError, match='float32'):
        sst_amd.crop_tracklet_points([trk()], {T.TS0: np.zeros((4, 3), np.float64)}, 1)
    unfrozen = sst_amd.LiDARTracklet('s', 'u', 1, True, torch.zeros(1, 7), [T.TS0], [0.5])
    with pytest.raises(RuntimeError, match='frozen'):
        sst_amd.tracklet_affinity([unfrozen], [trk()])
    other = trk()
    other.in_world = False
    with pytest.raises(AssertionError, match='in_world'):
        sst_amd.tracklet_affinity([trk()], [other])
    with pytest.raises(AssertionError):
        trk().max_iou(other)
    # no ground truth in the segment: nothing to launch, the reference's empty list
    assert sst_amd.generate_candidates([trk(seg='x')], [trk(seg='y')], 0.5) == [[]]


def test_cpu_tensors_are_refused(gold):
    import sst_amd
    pd, gt = P.gold_scene(gold)
    lp, lg = [P.lidar(t) for t in pd], [P.lidar(t) for t in gt]
    with pytest.raises(RuntimeError, match='no CPU path'):
        sst_amd.tracklet_affinity(lp, lg, device='cpu')
    with pytest.raises(RuntimeError, match='no CPU path'):
        sst_amd.generate_candidates(lp, lg, 0.5, device='cpu')
    with pytest.raises(RuntimeError, match='no CPU path'):
        sst_amd.box_point_crops([torch.zeros(5, 3)], [torch.zeros(1, 7)])
    with pytest.raises(RuntimeError, match='no CPU path'):
        sst_amd.box_point_counts([torch.zeros(5, 3)], [torch.zeros(1, 7)])
    with pytest.raises(RuntimeError, match='no CPU path'):
        sst_amd.remove_empty_boxes([torch.zeros(1, 7)], [torch.zeros(5, 3)], 0.2, 0.0)
    trks, frames = P.gold_crop_scene(gold)
    with pytest.raises(RuntimeError, match='no CPU path'):
        sst_amd.crop_tracklet_points([P.lidar(t) for t in trks], frames, 1, device='cpu')


@pytest.mark.parametrize('name', ['extend', 'extend_all'])
def test_track_extension_is_still_refused_by_name(gold, name):
    pd, _ = P.gold_scene(gold)
    with pytest.raises(NotImplementedError, match=name):
        getattr(P.lidar(pd[0]), name)()
