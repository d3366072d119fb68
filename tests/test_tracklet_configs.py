"""The CTRL family's modules without a GPU: the three shipped configs (tests/golden/configs/ctrl, resolved by
tests/golden/make_ctrl_fixtures.py) construct through the registry and equal the config text where the reference exists, the
state_dict keys equal the reference's (stored in tests/golden/tracklet_train.npz; the new modules own no parameter), every refused
setting raises by name, and the host-side halves of TrackletRoIHead (tracklets2rois, get_gt_rois) equal the reference's results
(tests/golden/tracklet_train.npz)."""
import copy
import glob
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

import tracklet_ref as T
from test_configs_build import FIXTURES, REF, load_config

NAMES = ('ctrl_veh_24e', 'ctrl_ped_24e', 'ctrl_cyc_12e')


def fixture(name):
    return eval(open(os.path.join(FIXTURES, 'ctrl', name + '.model.py')).read())


def test_the_three_shipped_configs_have_fixtures():
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(FIXTURES, 'ctrl', '*.model.py'))) == sorted(n + '.model.py' for n in NAMES)


@pytest.mark.parametrize('name', NAMES)
def test_fixture_equals_the_config_text(name):
    path = os.path.join(REF, 'configs', 'ctrl', name + '.py')
    if not os.path.exists(path):
        pytest.skip('the reference tree is not on this machine')
    assert load_config(path)['model'] == fixture(name)


@pytest.mark.parametrize('name', NAMES)
def test_config_constructs_through_the_registry(name):
    import sst_amd
    model = fixture(name)
    det = sst_amd.build_detector(copy.deepcopy(model))
    assert isinstance(det, sst_amd.TrackletDetector) and isinstance(det.segmentor, sst_amd.TrackletSegmentor)
    assert isinstance(det.roi_head, sst_amd.TrackletRoIHead) and isinstance(det.roi_head.roi_extractor, sst_amd.TrackletPointRoIExtractor)
    assert not hasattr(det.segmentor, 'segmentation_head') and det.roi_head.with_roi_scores and det.roi_head.roi_extractor.combined
    assert det.roi_head.roi_extractor.max_all_point == (300000, 600000) and det.roi_head.bbox_head.num_blocks == 6
    # the parameters are those of the modules that exist already, under the reference's attribute names
    keys = list(det.state_dict())
    vfe = sst_amd.build_voxel_encoder(copy.deepcopy(model['segmentor']['voxel_encoder']))
    unet = sst_amd.build_backbone(copy.deepcopy(model['segmentor']['backbone']))
    head = sst_amd.build_head(dict(copy.deepcopy(model['roi_head']['bbox_head']), train_cfg=model['train_cfg'], test_cfg=model['test_cfg']))
    expected = (['segmentor.voxel_encoder.' + k for k in vfe.state_dict()] + ['segmentor.backbone.' + k for k in unet.state_dict()]
                + ['roi_head.bbox_head.' + k for k in head.state_dict()])
    assert keys == expected
    # ... and they are the reference's (its three parameter-owning modules built from the same config; the order inside a SIR layer
    # differs, as it does for every SIRLayer of this library: load_state_dict goes by name)
    assert sorted(keys) == sorted(load_golden('tracklet_train.npz')['state_keys_' + name].tolist())
    assert len(keys) > 300 and not any(k.startswith(('roi_head.roi_extractor.', 'segmentor.timestamp_encoder.')) for k in keys)
    with pytest.raises(NotImplementedError, match='get_bboxes_from_tracklet'):
        det.roi_head.bbox_head.get_bboxes_from_tracklet()


def small_roi_head(**over):
    model = fixture('ctrl_veh_24e')
    cfg = copy.deepcopy(model['roi_head'])
    cfg['bbox_head'].update(num_blocks=1, in_channels=[85], feat_channels=[[16, 16]], rel_mlp_hidden_dims=[[8, 8]], rel_mlp_in_channels=[13],
                            reg_mlp=[16], cls_mlp=[16])
    train_cfg, test_cfg = copy.deepcopy(model['train_cfg']), copy.deepcopy(model['test_cfg'])
    for k, v in over.items():
        where, key = k.split('__')
        dict(general=cfg['general_cfg'], train=train_cfg, test=test_cfg)[where][key] = v
    import sst_amd
    return sst_amd.build_head(dict(cfg, train_cfg=train_cfg, test_cfg=test_cfg))


@pytest.mark.parametrize('setting,word', [('general__with_roi_corners', 'with_roi_corners'), ('general__checkpointing', 'checkpointing'),
                                          ('train__merge_candidates', 'merge_candidates'), ('test__tta', 'tta')])
def test_roi_head_refuses_by_name(setting, word):
    with pytest.raises(NotImplementedError, match=word):
        small_roi_head(**{setting: dict(merge='max') if word == 'tta' else True})
    assert small_roi_head() is not None


def test_detector_and_segmentor_refuse_by_name():
    import sst_amd
    model = fixture('ctrl_veh_24e')
    for where, key, value in (('train_cfg', 'pre_voxelization_size', (0.1, 0.1, 0.1)), ('test_cfg', 'tta', dict(merge='weighted'))):
        bad = copy.deepcopy(model)
        bad[where][key] = value
        with pytest.raises(NotImplementedError, match=key):
            sst_amd.build_detector(bad)
    with pytest.raises(NotImplementedError, match='aug_test'):
        sst_amd.TrackletDetector.aug_test(None)
    with pytest.raises(NotImplementedError, match='aug_test'):
        sst_amd.TrackletSegmentor.aug_test(None)
    with pytest.raises(NotImplementedError, match='strategy'):
        sst_amd.TimestampEncoder(dict(strategy='sinusoid', normalizer=100))
    enc = sst_amd.TimestampEncoder(dict(strategy='scalar', normalizer=100))
    out = enc(torch.arange(12.).reshape(3, 4), torch.zeros(3, dtype=torch.long))
    assert out.shape == (3, 5) and torch.equal(out[:, 4], torch.tensor([3., 7., 11.]) / 100)


def test_extractor_caps_follow_the_mode():
    import sst_amd
    ext = sst_amd.TrackletPointRoIExtractor(max_all_point=(300, 600), combined=True)
    assert ext._cap() == 300 and ext.eval()._cap() == 600 and sst_amd.TrackletPointRoIExtractor(max_all_point=77)._cap() == 77


def test_rois_of_tracklets_equal_the_reference():
    import sst_amd
    gold = load_golden('tracklet_train.npz')
    trks, cand_lists = T.gold_scene(gold)

    def lidar(trk, name):
        t = sst_amd.LiDARTracklet('seg', name, int(trk.type), True, trk.boxes.clone(), list(trk.ts_list), list(trk.score_list))
        t.freeze()
        t.set_type(int(trk.type), 'mmdet3d')
        return t

    head = small_roi_head()
    lt = [lidar(t, str(i)) for i, t in enumerate(trks)]
    rois, roi_frame_inds, cls_preds, labels_3d = head.tracklets2rois(lt)
    assert np.array_equal(rois.numpy(), gold['oc1_rois_f64'].astype(np.float32))
    assert np.array_equal(roi_frame_inds.numpy(), gold['oc1_roi_frame_inds']) and np.array_equal(labels_3d.numpy(), gold['oc1_labels_3d'])
    assert np.array_equal(cls_preds.numpy(), gold['oc1_cls_preds_f64'].astype(np.float32))
    chosen = gold['oc1_chosen'].tolist()
    gts = [lidar(cand_lists[i][k], 'g') if k >= 0 else lt[i].new_empty() for i, k in enumerate(chosen)]
    gt_rois = head.get_gt_rois(lt, gts)
    assert np.array_equal(gt_rois.numpy(), gold['oc1_gt_rois_f64'].astype(np.float32))
