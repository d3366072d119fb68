"""VoteSegHead's training side without a GPU: the restatement of tests/seg_loss_ref.py against the reference's own methods
(tests/golden/seg_head_train.npz, and live where the reference tree is present), the loud failures of the Python entry
points, and the loss parsing of every shipped segmentor config."""
import ast
import glob
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden

import seg_loss_ref as R

WIDTHS = {'none': None, 'p02': 0.2, 'm03': -0.3}
WAYMO = dict(score_thresh=(0.3, 0.25, 0.25), gamma=3.0, alpha=0.8)


@pytest.fixture(scope='module')
def gold():
    return load_golden('seg_head_train.npz')


def _scene(gold, case):
    key = 'labels3' if case == 'sig' else 'labels10'
    return ([gold['points0'], gold['points1']], [gold['boxes0'], gold['boxes1']], [gold[f'{key}_0'], gold[f'{key}_1']],
            3 if case == 'sig' else 10)


def loss_kwargs(case):
    if case == 'sig':
        return dict(mode=R.SIGMOID_FOCAL, **WAYMO)
    return dict(mode=R.SOFTMAX_CE, class_weight=R.NUSC_CLASS_WEIGHT, score_thresh=R.NUSC_SCORE_THRESH,
                class_group=R.class_group(R.NUSC_CLASS_NAMES, R.NUSC_GROUP_NAMES))


def recall_names(case):
    return ['Car', 'Ped', 'Cyc'] if case == 'sig' else R.NUSC_CLASS_NAMES


@pytest.mark.parametrize('case', ['sig', 'ce'])
@pytest.mark.parametrize('tag', list(WIDTHS))
def test_restated_targets_equal_the_reference(gold, case, tag):
    points, boxes, labels, bg = _scene(gold, case)
    lab, tgt, mask, inbox = R.point_targets(points, boxes, labels, bg, WIDTHS[tag])
    assert np.array_equal(lab, gold[f'tgt_{case}_{tag}_labels'])
    assert np.array_equal(mask, gold[f'tgt_{tag}_mask'])
    assert np.array_equal(inbox >= 0, mask)
    # torch's CPU sqrt / pow(0.5) is itself off by one ulp on some inputs: the contract is the correctly rounded root
    assert R.ulp_distance(tgt, gold[f'tgt_{tag}_targets']).max() <= 1
    # and the float64 run of the reference is the value the float32 one rounds
    assert np.abs(tgt.astype(np.float64) - gold[f'tgt_{tag}_targets64']).max() < 2e-6
    assert mask.sum() > 50 and (~mask).sum() > 100
    all_labels = np.concatenate(labels)
    assert not (mask & (all_labels[np.clip(inbox, 0, None)] < 0)).any(), 'a box labelled -1 took a point'


def test_the_three_widths_give_different_targets(gold):
    masks = [gold[f'tgt_{tag}_mask'] for tag in WIDTHS]
    assert masks[1].sum() > masks[0].sum() > masks[2].sum()
    # the 0.5 m wide box keeps its own extents at extra_width -0.3: its points stay
    points, boxes, labels, bg = _scene(gold, 'sig')
    inbox = R.point_targets(points, boxes, labels, bg, -0.3)[3]
    assert (inbox == 2).sum() > 0


@pytest.mark.parametrize('case', ['sig', 'ce'])
def test_restated_losses_equal_the_reference_in_float64(gold, case):
    logits = torch.from_numpy(gold[f'{case}_logits'].astype(np.float32))
    votes = torch.from_numpy(gold[f'{case}_vote_preds'].astype(np.float32))
    lab = torch.from_numpy(gold[f'tgt_{case}_none_labels'])
    tgt = torch.from_numpy(gold['tgt_none_targets'])
    mask = torch.from_numpy(gold['tgt_none_mask'])
    out = R.losses_and_grads(logits, votes, lab, tgt, mask, **loss_kwargs(case))
    assert abs(out['loss_sem'] - float(gold[f'{case}_f64_loss_sem_seg'][0])) <= 1e-12 * abs(out['loss_sem'])
    assert abs(out['loss_vote'] - float(gold[f'{case}_f64_loss_vote'][0])) <= 1e-12 * abs(out['loss_vote'])
    for name, key in (('d_logits', 'd_logits'), ('d_vote_preds', 'd_vote_preds')):
        ref = gold[f'{case}_f64_{key}']
        assert np.abs(out[name].numpy() - ref).max() <= 1e-12 * np.abs(ref).max()
    assert out['status'] == 0 and out['num_valid'] == int(mask.sum()) and out['margin'] > 5e-5
    for k, name in enumerate(recall_names(case)):
        assert float(out['recall'][k]) == float(gold[f'{case}_f32_recall_{name}'][0])
    if case == 'ce':
        assert out['num_fg'] == int(gold['ce_f32_num_fg'][0]) == int(gold['ce_f64_num_fg'][0])
    # the stored noise is what the tolerances of the GPU tests are built from: it has the size the issue measured
    for key in ('loss_sem_seg', 'loss_vote', 'd_logits', 'd_vote_preds'):
        assert 0 <= float(gold[f'noise_{case}_{key}'].max()) < 1e-6


def _have_reference():
    from oracle import build_ref, ref_loader
    return ref_loader.available() and build_ref.load_points_in_boxes() is not None


def test_restatement_equals_the_live_reference_on_fresh_data():
    if not _have_reference():
        pytest.skip('reference tree / compiled points_in_boxes_cpu not present')
    sys.path.insert(0, GOLDEN)
    import make_seg_head_train as M
    rng = np.random.default_rng(7)
    boxes = [M.make_boxes(rng, 6, np.float32([3, -4])), M.make_boxes(rng, 5, np.float32([30, 20]))]
    points = [M.make_points(rng, boxes[0], 150), M.make_points(rng, boxes[1], 120)]
    labels = [np.array([1, 0, 2, -1, 2, 0], np.int64), np.array([0, -1, 1, -1, 2], np.int64)]
    n = 270
    for width in (None, 0.2, -0.3):
        head = M.make_head(True, 3, {} if width is None else {'extra_width': width}, logit_scale=0.5, gamma=2.0, alpha=0.25,
                           w_decode=1.0)
        head.train_cfg.update(score_thresh=(0.3, 0.25, 0.25), class_names=('Car', 'Ped', 'Cyc'))
        lab, tgt, mask = M.reference_targets(head, [p[:, :3] for p in points], boxes, labels)
        rlab, rtgt, rmask, _ = R.point_targets(points, boxes, labels, 3, width)
        assert np.array_equal(lab, rlab) and np.array_equal(mask, rmask)
        assert R.ulp_distance(tgt, rtgt).max() <= 1
    logits = rng.normal(0, 2, (n, 3)).astype(np.float32)
    votes = rng.normal(0, 1, (n, 9)).astype(np.float32)
    ref = M.reference_losses(head, logits, votes, lab, tgt, mask, torch.float64)
    out = R.losses_and_grads(torch.from_numpy(logits), torch.from_numpy(votes), torch.from_numpy(lab),
                             torch.from_numpy(tgt), torch.from_numpy(mask), R.SIGMOID_FOCAL, logit_scale=0.5, gamma=2.0,
                             alpha=0.25)
    assert abs(out['loss_sem'] - float(ref['loss_sem_seg'][0])) <= 1e-12 * abs(out['loss_sem'])
    assert abs(out['loss_vote'] - float(ref['loss_vote'][0])) <= 1e-12
    assert np.abs(out['d_logits'].numpy() - ref['d_logits']).max() <= 1e-12 * np.abs(ref['d_logits']).max()
    assert np.abs(out['d_vote_preds'].numpy() - ref['d_vote_preds']).max() <= 1e-12


def test_python_entry_points_fail_loudly_on_cpu_tensors():
    import sst_amd
    pts, boxes, labels = torch.zeros(5, 4), torch.zeros(2, 7), torch.zeros(2, dtype=torch.long)
    with pytest.raises(RuntimeError):
        sst_amd.seg_point_targets([pts], [boxes], [labels], 3)
    with pytest.raises(RuntimeError):
        sst_amd.seg_vote_loss(torch.zeros(5, 3), torch.zeros(5, 9), torch.zeros(5, dtype=torch.long), torch.zeros(5, 3),
                              torch.zeros(5, dtype=torch.bool), mode=sst_amd.seg_loss.SIGMOID_FOCAL)
    with pytest.raises(RuntimeError):
        sst_amd.seg_vote_loss(torch.zeros(5, 3), torch.zeros(5, 9), torch.zeros(5, dtype=torch.long), torch.zeros(5, 3),
                              torch.zeros(5, dtype=torch.bool), mode=7)


def test_capi_refuses_bad_arguments_without_launching():
    from sst_amd import _lib
    lib = _lib.load()
    assert lib.sst_seg_targets_box_tile() >= 64 and lib.sst_seg_loss_tile_rows() >= 64
    assert lib.sst_seg_loss_workspace_bytes(1, 3) >= 11 * 8
    t = lib.sst_seg_loss_tile_rows()
    assert lib.sst_seg_loss_workspace_bytes(2 * t + 1, 3) >= 3 * 11 * 8
    null = [None] * 5
    assert lib.sst_seg_loss_fwd_f32(*null, 10, 3, 0, 1.0, 2.0, 0.25, None, None, None, 0, None, None, None, None) \
        == _lib.SST_ERR_ARG
    assert lib.sst_seg_loss_bwd_f32(*null, 0, 3, 0, 1.0, 2.0, 0.25, None, None, None, None, None, None) == _lib.SST_ERR_ARG
    assert lib.sst_seg_targets_f32(None, 3, 10, None, 1, None, None, None, 0, 0, 0.0, 3, None, None, None, None, None,
                                   None) == _lib.SST_ERR_ARG
    # shape / mode refusals come after the pointer checks: hand in non-null (never dereferenced) addresses
    import ctypes
    buf = ctypes.create_string_buffer(64)
    p = [ctypes.cast(buf, ctypes.c_void_p)] * 5
    assert lib.sst_seg_loss_fwd_f32(*p, 10, 33, 0, 1.0, 2.0, 0.25, None, None, None, 0, p[0], p[0], p[0], None) \
        == _lib.SST_ERR_UNSUPPORTED
    assert lib.sst_seg_loss_fwd_f32(*p, 10, 0, 0, 1.0, 2.0, 0.25, None, None, None, 0, p[0], p[0], p[0], None) \
        == _lib.SST_ERR_UNSUPPORTED
    assert lib.sst_seg_loss_fwd_f32(*p, 10, 3, 2, 1.0, 2.0, 0.25, None, None, None, 0, p[0], p[0], p[0], None) \
        == _lib.SST_ERR_UNSUPPORTED
    assert lib.sst_seg_loss_bwd_f32(*p, 10, 3, 5, 1.0, 2.0, 0.25, None, p[0], p[0], p[0], p[0], None) \
        == _lib.SST_ERR_UNSUPPORTED


def _segmentor_blocks():
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, 'configs', 'fsd*', '*.model.py'))):
        model = ast.literal_eval(open(path).read())
        seg = model['segmentor'] if 'segmentor' in model else model
        assert seg['type'] == 'VoteSegmentor', path
        out.append((os.path.relpath(path, GOLDEN), seg))
    return out


def test_vote_seg_head_constructs_from_every_shipped_config_and_reports_its_loss_mode():
    from sst_amd.detectors import build_head
    blocks = _segmentor_blocks()
    assert len(blocks) >= 10
    modes = set()
    for name, seg in blocks:
        cfg = seg['segmentation_head']
        head = build_head(dict(cfg))
        assert head.loss_unbuilt == [], (name, head.loss_unbuilt)
        want = 'sigmoid_focal' if cfg['loss_decode']['type'] == 'FocalLoss' else 'softmax_ce'
        assert head.loss_mode == want, name
        assert head.loss_args['loss_weight_decode'] == cfg['loss_decode']['loss_weight']
        if want == 'sigmoid_focal':
            assert (head.loss_args['gamma'], head.loss_args['alpha']) == (cfg['loss_decode']['gamma'], cfg['loss_decode']['alpha'])
            assert head.num_classes == cfg['num_classes'] == head.bg_label
        else:
            assert head.loss_args['class_weight'] == cfg['loss_decode']['class_weight']
            assert head.num_classes == cfg['num_classes'] + 1
        modes.add(head.loss_mode)
    assert modes == {'sigmoid_focal', 'softmax_ce'}


def test_unbuilt_losses_construct_and_refuse_only_when_called():
    from sst_amd.detectors import VoteSegHead
    for kw in (dict(loss_aux=dict(type='LovaszLoss', loss_weight=1.0)),
               dict(loss_decode=dict(type='DiceLoss')),
               dict(loss_vote=dict(type='SmoothL1Loss', beta=0.1))):
        args = dict(loss_decode=dict(type='FocalLoss', use_sigmoid=True, gamma=3.0, alpha=0.8, loss_weight=1.0),
                    loss_vote=dict(type='L1Loss', loss_weight=1.0))
        args.update(kw)
        head = VoteSegHead(in_channel=16, num_classes=3, hidden_dims=[], dropout_ratio=0.0, **args)
        assert head.loss_unbuilt
        with pytest.raises(NotImplementedError):
            head.losses(torch.zeros(4, 3), torch.zeros(4, 9), torch.zeros(4, dtype=torch.long), torch.zeros(4, 3),
                        torch.zeros(4, dtype=torch.bool))
