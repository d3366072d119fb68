"""The FSD++ family without a GPU: the shipped config (tests/golden/configs/fsdpp, resolved by tests/golden/make_fsdpp_fixtures.py)
constructs through the registry as TwoStageFSDPP, its state_dict keys equal those of the same dictionary built as FSD (the stage
owns no parameter), the fixture equals the config text where the reference exists, every refused setting raises by name, and
simple_test without reuse_test raises as the reference does."""
import copy
import glob
import os

import pytest
import torch

from test_configs_build import FIXTURES, REF, load_config

NAME = 'fsdpp_waymoD1_1x_7f_6base'


def fixture():
    return eval(open(os.path.join(FIXTURES, 'fsdpp', NAME + '.model.py')).read())


def test_the_shipped_config_has_a_fixture():
    assert [os.path.basename(p) for p in glob.glob(os.path.join(FIXTURES, 'fsdpp', '*.model.py'))] == [NAME + '.model.py']


def test_fixture_equals_the_config_text():
    path = os.path.join(REF, 'configs', 'fsdpp', NAME + '.py')
    if not os.path.exists(path):
        pytest.skip('the reference tree is not on this machine')
    assert load_config(path)['model'] == fixture()


def test_config_constructs_through_the_registry():
    import sst_amd
    model = fixture()
    det = sst_amd.build_detector(copy.deepcopy(model))
    assert type(det).__name__ == 'TwoStageFSDPP' and isinstance(det, sst_amd.FSD)
    assert det.max_pre_frames == 6 and det.incremental_cfg['max_crop_points'] == 128 and det.rcnn_type == 'GroupCorrectionHead'
    assert det.previous_pc == [] and det.previous_pose == [] and det.previous_seed_info == [] and det.previous_cropped_pc == []
    assert det.frame_counter == 0 and det.last_segind == 'None'
    as_fsd = copy.deepcopy(model)
    as_fsd['type'] = 'FSD'
    as_fsd.pop('incremental_cfg')
    plain = sst_amd.build_detector(as_fsd)
    assert list(det.state_dict()) == list(plain.state_dict()) and len(det.state_dict()) > 200
    det.attach_heads()
    plain.attach_heads()
    assert list(det.state_dict()) == list(plain.state_dict())
    # the segmentor takes the frame id column: 5 point columns + 1
    assert model['segmentor']['voxel_encoder']['in_channels'] == 6 and model['segmentor']['tanh_dims'] == [3, 4]


@pytest.mark.parametrize('key,value', [('n_fps', 64), ('voxel_pooling_size', (0.1, 0.1, 0.1)), ('crop_painting', True),
                                       ('virtual_seed_points_cfg', dict(padding_dim=3)), ('noise_cfg', dict(drop_rate=0.1)),
                                       ('pre_nms_thr', 0.5), ('elegant_max_age', True)])
def test_incremental_cfg_refuses_by_name(key, value):
    import sst_amd
    bad = fixture()
    bad['incremental_cfg'][key] = value
    with pytest.raises(NotImplementedError, match=key):
        sst_amd.build_detector(bad)
    with pytest.raises(NotImplementedError, match=key):
        sst_amd.generate_points([], [], [], bad['incremental_cfg'], True)


def test_detector_refuses_by_name():
    import sst_amd
    bad = fixture()
    bad['roi_head']['type'] = 'IncrementalROIHead'
    with pytest.raises(NotImplementedError, match='IncrementalROIHead'):
        sst_amd.build_detector(bad)
    with pytest.raises(NotImplementedError, match='aug_test'):
        sst_amd.TwoStageFSDPP.aug_test(None)
    quiet = fixture()
    quiet['incremental_cfg'].update(pre_nms_thr=0, elegant_max_age=False, crop_painting=False, disable_incremental=True)
    assert sst_amd.build_detector(quiet) is not None


def test_simple_test_without_reuse_test_raises():
    import sst_amd
    model = fixture()
    model['test_cfg']['reuse_test'] = False
    det = sst_amd.build_detector(model).eval()
    seed = [[[dict(gt_bboxes_3d=torch.zeros(0, 7), gt_labels_3d=torch.zeros(0), scores=torch.zeros(0))]]]
    with pytest.raises(NotImplementedError, match='LoadPreviousFramesWaymo'):
        det.simple_test([torch.zeros(4, 5)], [dict(sample_idx=1000000)], seed_info=seed, pose=[torch.eye(4)])


def test_preprocess_seed_filters_scores_and_cuts_frames():
    import numpy as np
    import sst_amd
    model = fixture()
    model['incremental_cfg'].update(pre_score_thr=0.5, num_previous_frames=2)
    det = sst_amd.build_detector(model).train()
    frame = dict(gt_bboxes_3d=torch.arange(21.).reshape(3, 7), gt_labels_3d=np.asarray([0, 1, 2]), scores=np.asarray([0.9, 0.5, 0.6], np.float32))
    empty = dict(gt_bboxes_3d=torch.zeros(0, 7), gt_labels_3d=np.zeros(0), scores=np.zeros(0, np.float32))
    out = det.preprocess_seed([[frame, empty, frame]])
    assert len(out) == 1 and len(out[0]) == 2
    assert out[0][0]['gt_bboxes_3d'].tolist() == frame['gt_bboxes_3d'][[0, 2]].tolist()
    assert out[0][0]['gt_labels_3d'].tolist() == [0, 2] and out[0][1] is empty
