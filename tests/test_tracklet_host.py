"""The CTRL tracklet family without a GPU: the torch restatement of the targets (tests/tracklet_ref.py) against the reference's own
results (tests/golden/tracklet_train.npz), the host methods of sst_amd.LiDARTracklet against the same file, the refusals, and the
header / binding consistency of the new entry points.  Integers, orders and chosen candidates match exactly; float64 restatement
within the reference's own float32-vs-float64 gap, float32 within max(4 x that gap, 1e-6) (relative to the largest element)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

import tracklet_ref as T

EXACT = ('chosen', 'assigned_gt_inds', 'frame_inds', 'counts', 'reg_mask', 'labels')


@pytest.fixture(scope='module')
def gold():
    return load_golden('tracklet_train.npz')


def test_argmax_of_the_host_counts_is_the_first_maximum():
    """_select_one2one_candidates takes torch.argmax of an int64 host tensor: the first of equal maxima"""
    assert int(torch.argmax(torch.tensor([2, 5, 5, 1]))) == 1
    assert int(torch.argmax(torch.tensor([torch.tensor(3), torch.tensor(3), torch.tensor(3)]))) == 0
    assert int(torch.argmax(torch.tensor([0, 0]))) == 0


@pytest.mark.parametrize('oc', [0, 1])
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_restatement_equals_the_reference(gold, oc, dtype):
    trks, cand_lists = T.gold_scene(gold)
    res = T.targets(trks, cand_lists, dict(T.GOLD_CFG, object_centric=bool(oc)), dtype)
    for k in EXACT:
        assert np.array_equal(res[k].numpy().astype(np.int64), gold[f'oc{oc}_{k}'].astype(np.int64)), k
    assert int(res['chosen'][3]) == 0 and int(res['chosen'][4]) == 2 and int(res['chosen'][1]) == -1      # the tie, the last, none
    for k in ('iou', 'soft_label', 'targets'):
        gap = float(gold[f'noise_oc{oc}_{k}'])
        err = T.rel_err(res[k].numpy(), gold[f'oc{oc}_{k}_f64'])
        limit = max(gap, 1e-12) if dtype == torch.float64 else T.bar(gap)
        print(k, dtype, 'err', err, 'gap', gap)
        assert err <= limit, (k, err, limit)


def lidar(trk, name='t', poses=None):
    import sst_amd
    t = sst_amd.LiDARTracklet('seg', name, int(trk.type), True, trk.boxes.clone(), list(trk.ts_list), list(trk.score_list))
    t.freeze()
    if poses is not None:
        t.pose_list = [torch.as_tensor(p, dtype=torch.float32) for p in poses]
    return t


def host_tracklet(gold):
    return lidar(T.Trk(gold['host_boxes'], gold['host_ts'].tolist(), gold['host_scores'].tolist(), 0), 'h', gold['host_poses'])


def close(got, gold, key):
    err = T.rel_err(got, gold[f'host_{key}_f64'])
    print(key, 'err', err, 'gap', float(gold[f'noise_host_{key}']))
    assert err <= T.bar(gold[f'noise_host_{key}']), (key, err)


def test_tracklet_geometry_equals_the_reference(gold):
    for key, call in (('flip_h', lambda t: t.flip('horizontal')), ('flip_v', lambda t: t.flip('vertical')),
                      ('rotate', lambda t: t.rotate(0.37)), ('translate', lambda t: t.translate([1.5, -2.0, 0.25])),
                      ('scale', lambda t: t.scale(1.1))):
        t = host_tracklet(gold)
        call(t)
        close(t.concated_boxes().numpy(), gold, key)
        assert t.box_list[3].data_ptr() == t.boxes[3:4].data_ptr()      # box_list are row views of the one tensor


def test_frame_transform_shared2ego_and_update_equal_the_reference(gold):
    t = host_tracklet(gold)
    t.frame_transform(torch.as_tensor(gold['host_shared_pose'], dtype=torch.float32))
    close(t.concated_boxes().numpy(), gold, 'frame_transform')
    close(t.shared2ego().numpy(), gold, 'shared2ego')
    n = len(t)
    t.update_from_prediction(torch.as_tensor(gold['host_new_boxes']), torch.as_tensor(gold['host_new_scores']),
                             torch.zeros(n, dtype=torch.long), torch.as_tensor(gold['host_valid']))
    close(t.concated_boxes().numpy(), gold, 'updated_boxes')
    assert np.array_equal(np.asarray(t.score_list, np.float32), gold['host_updated_scores_f64'].astype(np.float32))
    assert t.pose_list is None and not bool(gold['host_valid'][1])        # an invalid RoI keeps the old box and score
    assert t.score_list[1] == pytest.approx(float(gold['host_scores'][1]))


def test_timestamp_methods_equal_the_reference(gold):
    t = host_tracklet(gold)
    o = lidar(T.Trk(gold['host_other_boxes'], gold['host_other_ts'].tolist(), [1.0] * len(gold['host_other_ts']), 0), 'o')
    assert t.ts_intersection(o) == gold['host_ts_intersection'].tolist()
    assert [o.get_index_from_ts(x) for x in t.ts_list] == gold['host_index_from_ts'].tolist()
    boxes, mask = o.concated_boxes_from_ts(t.ts_list)
    assert np.array_equal(mask.numpy(), gold['host_mask_from_ts'])
    assert np.array_equal(boxes.numpy(), gold['host_boxes_from_ts_f64'].astype(np.float32))
    e = t.new_empty()
    assert len(e) == 0 and e.id == 'h_empty' and e.concated_boxes().shape == (0, 7) and e.ts_intersection(t) == []
    b, m = e.concated_boxes_from_ts(t.ts_list)
    assert b.shape == (len(t), 7) and not m.any()
    assert t[t.ts_list[2]].data_ptr() == t.boxes[2:3].data_ptr() and t[10 ** 16] is None and t[2].shape == (1, 7)
    with pytest.raises(KeyError):
        t[len(t)]


def test_dump_and_collate_formats_round_trip(gold):
    import sst_amd
    t = host_tracklet(gold)
    d = t.to_dump_format()
    assert d[0] == 'seg' and d[1] == 'h' and len(d[4]) == len(t) and d[4][0].shape == (1, 7)
    back = sst_amd.LiDARTracklet.from_dump_format(d)
    assert back.frozen and torch.equal(back.boxes, t.boxes) and back.ts_list == t.ts_list and back.uuid == t.uuid
    t.to_collate_format()
    assert isinstance(t.boxes, np.ndarray) and isinstance(t.pose_list[0], np.ndarray)
    t.from_collate_format()
    assert torch.equal(t.boxes, back.boxes) and torch.is_tensor(t.pose_list[0])
    m = host_tracklet(gold)
    o = lidar(T.Trk(gold['host_other_boxes'], gold['host_other_ts'].tolist(), [0.5] * len(gold['host_other_ts']), 0), 'o',
              gold['host_poses'][:len(gold['host_other_ts'])])
    m.merge_not_exist(o)
    assert len(m) == len(t) + 2 and m.ts_list[-2:] == gold['host_other_ts'][-2:].tolist() and torch.equal(m.boxes[:len(t)], back.boxes)
    assert torch.equal(m.boxes[-2:], o.boxes[-2:]) and m.score_list[-1] == 0.5 and len(m.pose_list) == len(m)


@pytest.mark.parametrize('name', ['merge_augs', 'extend', 'extend_all', 'add_center_noise', 'add_size_noise', 'add_yaw_noise',
                                  'random_frame_drop'])
def test_pipeline_methods_are_refused_by_name(gold, name):
    t = host_tracklet(gold)
    with pytest.raises(NotImplementedError, match=name):
        getattr(t, name)()


def test_targets_refuse_by_name_and_without_a_gpu(gold):
    import sst_amd
    trks, cand_lists = T.gold_scene(gold)
    lt = [lidar(t, str(i)) for i, t in enumerate(trks)]
    lc = [[lidar(c, 'c') for c in cs] for cs in cand_lists]
    with pytest.raises(NotImplementedError, match='merge_candidates'):
        sst_amd.tracklet_targets(lt, lc, dict(T.GOLD_CFG, merge_candidates=True))
    with pytest.raises(RuntimeError, match='no CPU path'):
        sst_amd.tracklet_targets(lt, lc, T.GOLD_CFG, device='cpu')
    with pytest.raises(RuntimeError):
        sst_amd.tracklet_rows(torch.zeros(4, 8), torch.zeros(4, 3), torch.zeros(4, dtype=torch.long), torch.zeros(2, dtype=torch.long),
                              torch.zeros(2, dtype=torch.long), torch.zeros(1, dtype=torch.long))


@pytest.mark.parametrize('struct,cname', [('TrackletTargetsArgs', 'sst_tracklet_targets_args'),
                                          ('TrackletRowsArgs', 'sst_tracklet_rows_args')])
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


def test_library_answers_the_launch_constant_without_a_gpu():
    from sst_amd import _lib
    assert _lib.load().sst_tracklet_targets_block() == 256
    assert _lib.load().sst_tracklet_targets_f32(None, None) == _lib.SST_ERR_ARG
    assert _lib.load().sst_tracklet_rows_fwd_f32(None, None) == _lib.SST_ERR_ARG
    assert _lib.load().sst_tracklet_rows_bwd_f32(None, -1, 0, 0, None, 0, None, None) == _lib.SST_ERR_ARG
    assert _lib.load().sst_tracklet_rows_keys_i64(None, 5, 5, None, None) == _lib.SST_ERR_ARG
