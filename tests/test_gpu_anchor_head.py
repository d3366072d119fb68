"""Anchor3DHead's targets, losses and decoding on the GPU (csrc/anchor_head.hip) against the reference's golden
(tests/golden/anchor_head_train.npz) and the restatement of tests/anchor_head_ref.py.

Targets: ``assigned`` equals the golden and the restatement exactly, the per-box maxima are bit-equal to the restatement's (the
restatement runs on the device's own centre tables copied to the host, which are also checked against the reference's anchors bit
for bit).  anchor_target_3d: integers and weights exactly, the plain target columns bit for bit, the log columns within ULP_MATH.
Decoding: columns built from exact operations (x, y, yaw) bit for bit, exp and sigmoid within ULP_MATH, z within what the height's
ULP_MATH allows (z = zt * ha + za - hg / 2); kept sets, their order and labels exactly the golden's.

ULP_MATH = 2 by the argument at the top of tests/test_gpu_center_head.py: both sides' log / exp are within 1 ulp of the true value.

Losses (float64 autograd of the restatement on the same float32 inputs): relative error of each loss scalar and
max |err| / max |grad| of each gradient tensor <= max(4 * noise, 1e-6), noise = the reference's own float32-vs-float64 gap stored
in the golden; cases without a golden use the floor alone.  Every case prints its errors before it asserts (pytest -s)."""
import ast
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

import anchor_head_ref as R

DEV = 'cuda:0'
ULP_MATH = 2
NAMES = ('labels', 'label_weights', 'bbox_targets', 'bbox_weights', 'dir_targets', 'dir_weights')


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


@pytest.fixture(scope='module')
def gold():
    return load_golden('anchor_head_train.npz')


def _scene(gold, case):
    sel = [R.case_labels(case, gold[f'labels{s}']) for s in range(3)]
    return [gold[f'boxes{s}'][k] for s, (k, _) in enumerate(sel)], [l[k] for k, l in sel]


def _head(cfg, channels=8):
    import sst_amd
    return sst_amd.build_head(dict(cfg, type='Anchor3DHead', in_channels=channels, feat_channels=channels)).to(DEV)


def _host_grid(grid):
    """the device's centre tables as the restatement's Grid"""
    return R.Grid(grid.xs.cpu().numpy(), grid.ys.cpu().numpy(), grid.zs.cpu().numpy(), np.float32(grid.sizes),
                  np.float32(grid.rotations))


_RESTATED = {}


def _restated(gold, case, grid):
    """the restated targets of a golden case on the device's tables, computed once and left unchanged"""
    if case not in _RESTATED:
        boxes, labels = _scene(gold, case)
        _RESTATED[case] = R.batch_targets(_host_grid(grid), boxes, labels, R.CASES[case])
    return _RESTATED[case]


def _check_compact(t, per_sample, what):
    assigned = t.assigned.cpu().numpy()
    want = np.stack([p[0].reshape(-1) for p in per_sample])
    print(f'{what}: anchors {assigned.shape}, positives {(assigned >= 0).sum(1)}, ignored {(assigned == -2).sum(1)}')
    assert assigned.dtype == np.int32 and np.array_equal(assigned, want), what
    gt_max = t.gt_max.cpu().numpy()
    want_max = np.concatenate([p[2] for p in per_sample], 1)
    assert np.array_equal(gt_max.view(np.int32), want_max.view(np.int32)), f'{what}: per-box maxima, bit for bit'
    assert t.pos_counts.cpu().tolist() == [int((p[0] >= 0).sum()) for p in per_sample], what


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(R.CASES))
def test_targets_equal_the_reference_and_the_restatement(gold, case):
    cfg = R.CASES[case]
    head = _head(cfg)
    boxes, labels = _scene(gold, case)
    gts, lbs = [_t(b) for b in boxes], [_t(l) for l in labels]
    t = head.targets(gts, lbs, (R.H, R.W))
    host = R.make_grid(cfg['anchor_generator'], R.H, R.W)
    dev = _host_grid(t.grid)
    for a, b in ((dev.xs, host.xs), (dev.ys, host.ys), (dev.zs, host.zs)):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), 'the centre tables are the reference\'s, bit for bit'
    if case == 'shipped':
        anchors = head.get_anchors([(R.H, R.W)], [None], device=DEV)[0][0]
        assert np.array_equal(anchors[0].cpu().numpy().view(np.int32), gold['anchors'].view(np.int32))
    dense, per_sample, n_pos, n_neg = _restated(gold, case, t.grid)
    assert np.array_equal(t.assigned.cpu().numpy(), gold[f'tgt_{case}_assigned'])
    _check_compact(t, per_sample, case)
    anchors = head.get_anchors([(R.H, R.W)], [None] * 3, device=DEV)
    out = head.anchor_target_3d(anchors, gts, [None] * 3, gt_labels_list=lbs, num_classes=cfg['num_classes'],
                                label_channels=head.cls_out_channels, sampling=False)
    assert (out[6], out[7]) == (int(gold[f'tgt_{case}_num_total_pos']), int(gold[f'tgt_{case}_num_total_neg'])) == (n_pos, n_neg)
    for k, lst in zip(NAMES, out[:6]):
        got, want = lst[0].cpu().numpy(), gold[f'tgt_{case}_{k}']
        assert len(lst) == 1 and got.dtype == want.dtype and got.shape == want.shape, k
        if k != 'bbox_targets':
            assert np.array_equal(got, want), k
            continue
        plain = [0, 1, 2, 6]
        assert np.array_equal(got[..., plain].view(np.int32), want[..., plain].view(np.int32)), 'plain target columns'
        d = R.ulp_distance(got[..., 3:6], want[..., 3:6]).max()
        print(f'{case}: log columns max ulp distance {d}')
        assert d <= ULP_MATH


def _sst_base():
    path = os.path.join(GOLDEN, 'configs', 'sst_refactor', 'sst_waymoD5_1x_3class_8heads_v2.model.py')
    return ast.literal_eval(open(path).read())


def _detector_like(rng, n, lo, hi, sizes=((2.08, 4.73, 1.77), (0.84, 1.81, 1.77), (0.84, 0.91, 1.74))):
    kind = rng.integers(0, len(sizes), n)
    b = np.zeros((n, 7), np.float32)
    b[:, :2] = rng.uniform(lo, hi, (n, 2))
    b[:, 3:6] = np.float32(sizes)[kind] * rng.uniform(0.8, 1.25, (n, 3))
    b[:, 2] = rng.uniform(-1.5, 0.0, n)
    b[:, 6] = rng.choice([0.0, np.pi / 2, np.pi, -np.pi / 2], n) + rng.normal(0, 0.3, n)
    return b, kind.astype(np.int64)


def _edge_scene(name):
    """-> (generator cfg, (H, W), boxes per sample, labels per sample, assign_per_class)"""
    import sst_amd
    rng = np.random.default_rng(11)
    empty = (np.zeros((0, 7), np.float32), np.zeros(0, np.int64))
    lo, hi = R.RANGE_XY[0] + 0.5, R.RANGE_XY[3] - 0.5
    chunk = sst_amd.anchor_head.targets_gt_chunk()
    if name == 'no_boxes':
        return R.generator_cfg(), (R.H, R.W), [empty, empty], False
    if name == 'one_box':
        return R.generator_cfg(), (R.H, R.W), [_detector_like(rng, 1, -2.0, 2.0), empty], False
    if name == 'chunk_plus_one':          # the chunk loop wraps; boxes crowd the map so that later chunks win anchors too
        return R.generator_cfg(), (R.H, R.W), [_detector_like(rng, chunk + 1, lo, hi), _detector_like(rng, 3, lo, hi)], True
    if name == 'ragged_map':              # 13 x 11 x 6 anchors: no multiple of the workgroup, one sample
        assert (13 * 11 * 6) % sst_amd.anchor_head.block_cells() != 0
        gen = dict(R.generator_cfg(), ranges=[[-3.52, -4.16, z, 3.52, 4.16, z] for z in (-0.0345, -0.1188, 0.0)])
        return gen, (13, 11), [_detector_like(rng, 9, -3.0, 3.0)], False
    assert name == 'launch'               # the shipped 468 x 468 map: 2 samples of at most 48 detector-like boxes
    gen = _sst_base()['bbox_head']['anchor_generator']
    return gen, (468, 468), [_detector_like(rng, 48, -74.0, 74.0), _detector_like(rng, 40, -30.0, 30.0)], False


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['no_boxes', 'one_box', 'chunk_plus_one', 'ragged_map', 'launch'])
def test_targets_at_the_shape_edges(name):
    import sst_amd
    gen_cfg, size, samples, per_class = _edge_scene(name)
    gen = sst_amd.build_anchor_generator(gen_cfg)
    t = sst_amd.anchor_targets([_t(b) for b, _ in samples], [_t(l) for _, l in samples], size, gen, R.ASSIGN_3, per_class)
    grid = _host_grid(t.grid)
    per_sample = [R.assign(grid, b, l, R.ASSIGN_3, per_class) for b, l in samples]
    _check_compact(t, per_sample, name)
    if name == 'no_boxes':
        assert (t.assigned == -1).all() and t.gt_max.numel() == 0
    if name == 'chunk_plus_one':
        assert (t.assigned[0] >= sst_amd.anchor_head.targets_gt_chunk()).sum() > 0, 'the box past the first chunk wins no anchor'
    if name == 'launch':
        assert (t.assigned >= 0).sum() > 100 and (t.assigned == -2).sum() > 100


def _gpu_losses(head, maps, gts, lbs):
    ts = [_t(m).requires_grad_(True) for m in maps]
    use_dir = head.use_direction_classifier
    out = head.loss([ts[0]], [ts[1]], [ts[2]] if use_dir else None, gts, lbs, [None] * len(gts))
    total = out['loss_cls'][0] + out['loss_bbox'][0] + (out['loss_dir'][0] if use_dir else 0)
    total.backward()
    res = dict(loss_cls=out['loss_cls'][0].item(), loss_bbox=out['loss_bbox'][0].item(),
               loss_dir=out['loss_dir'][0].item() if use_dir else 0.0)
    for k, t in zip(('d_cls', 'd_bbox', 'd_dir'), ts):
        res[k] = None if t.grad is None else t.grad.cpu().numpy()
    return res


def _check_losses(got, want, noise, what):
    report, ok = [], True
    for k in ('loss_cls', 'loss_bbox', 'loss_dir'):
        err = abs(got[k] - want[k]) / abs(want[k]) if want[k] != 0 else abs(got[k])
        tol = max(4 * noise.get(k, 0.0), 1e-6)
        report.append(f'{k} {err:.2e} (allowed {tol:.1e})')
        ok = ok and err <= tol
    for k in ('d_cls', 'd_bbox', 'd_dir'):
        if got[k] is None:
            continue
        scale = np.abs(want[k]).max()
        err = np.abs(got[k] - want[k]).max() / scale if scale > 0 else np.abs(got[k]).max()
        tol = max(4 * noise.get(k, 0.0), 1e-6)
        report.append(f'{k} {err:.2e} (allowed {tol:.1e})')
        ok = ok and err <= tol
    print(f'{what}: ' + ', '.join(report))
    assert ok, what


def _check_zero_gradients(got, assigned, n_a, c, hw_shape):
    """gradients of ignored anchors exactly 0; box and direction gradients of non-positive anchors exactly 0"""
    b = assigned.shape[0]
    h, w = hw_shape
    a = assigned.reshape(b, h, w, n_a)
    d_cls = got['d_cls'].reshape(b, n_a, c, h, w).transpose(0, 3, 4, 1, 2)
    assert (d_cls[a == -2] == 0).all() and (d_cls[a != -2] != 0).any()
    d_box = got['d_bbox'].reshape(b, n_a, 7, h, w).transpose(0, 3, 4, 1, 2)
    assert (d_box[a < 0] == 0).all() and (d_box[a >= 0] != 0).any()
    if got['d_dir'] is not None:
        d_dir = got['d_dir'].reshape(b, n_a, 2, h, w).transpose(0, 3, 4, 1, 2)
        assert (d_dir[a < 0] == 0).all() and (d_dir[a >= 0] != 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(R.CASES))
def test_losses_and_gradients_equal_the_reference(gold, case):
    cfg = R.CASES[case]
    head = _head(cfg)
    boxes, labels = _scene(gold, case)
    gts, lbs = [_t(b) for b in boxes], [_t(l) for l in labels]
    n_a, c = head.num_anchors, cfg['num_classes']
    maps = [gold[f'maps_{n_a}x{c}_{k}'].astype(np.float32) for k in ('cls', 'box', 'dir')]
    got = _gpu_losses(head, maps, gts, lbs)
    grid = _host_grid(head.anchor_generator.grid((R.H, R.W), DEV))
    dense64, per_sample, n_pos, _ = R.batch_targets(grid, boxes, labels, cfg, np.float64)
    want = R.loss_and_grads(*maps, dense64, n_pos, cfg)
    for k in ('loss_cls', 'loss_bbox', 'loss_dir'):
        assert abs(want[k] - float(gold[f'loss_{case}_f64_{k}'])) <= 1e-12 * abs(want[k])     # the restatement is the reference
    noise = {k: float(gold[f'noise_{case}_{k}']) for k in ('loss_cls', 'loss_bbox', 'loss_dir', 'd_cls', 'd_bbox', 'd_dir')}
    _check_losses(got, want, noise, case)
    _check_zero_gradients(got, np.stack([p[0].reshape(-1) for p in per_sample]), n_a, c, (R.H, R.W))
    again = _gpu_losses(head, maps, gts, lbs)
    for k, v in got.items():
        assert np.array_equal(np.asarray(v), np.asarray(again[k])), f'{k}: two runs differ'


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['no_direction_classifier', 'odd_map'])
def test_losses_without_a_golden(variant):
    rng = np.random.default_rng(3)
    if variant == 'no_direction_classifier':
        cfg = dict(R.CASES['per_class'], use_direction_classifier=False)
        size, samples = (R.H, R.W), [_detector_like(rng, 12, -6.0, 6.0), _detector_like(rng, 5, -6.0, 6.0)]
    else:       # 13 x 11 cells, one sample: the last workgroup is ragged; gamma and alpha off their defaults, smooth L1
        gen = dict(R.generator_cfg(), ranges=[[-3.52, -4.16, z, 3.52, 4.16, z] for z in (-0.0345, -0.1188, 0.0)])
        cfg = dict(R.CASES['smooth'], anchor_generator=gen, diff_rad_by_sin=True)
        size, samples = (13, 11), [_detector_like(rng, 9, -3.0, 3.0)]
    head = _head(cfg)
    n_a, c, b = head.num_anchors, cfg['num_classes'], len(samples)
    maps = [rng.normal(-2.0, 1.5, (b, n_a * c) + size).astype(np.float32), rng.normal(0, 0.3, (b, n_a * 7) + size).astype(np.float32),
            rng.normal(0, 1.0, (b, n_a * 2) + size).astype(np.float32)]
    boxes, labels = [s[0] for s in samples], [s[1] for s in samples]
    got = _gpu_losses(head, maps, [_t(x) for x in boxes], [_t(x) for x in labels])
    grid = _host_grid(head.anchor_generator.grid(size, DEV))
    dense64, per_sample, n_pos, _ = R.batch_targets(grid, boxes, labels, cfg, np.float64)
    use_dir = cfg['use_direction_classifier']
    want = R.loss_and_grads(maps[0], maps[1], maps[2] if use_dir else None, dense64, n_pos, cfg)
    assert sum((p[0] >= 0).sum() for p in per_sample) > 5
    if not use_dir:
        got['d_dir'] = None
    _check_losses(got, want, {}, variant)
    _check_zero_gradients(got, np.stack([p[0].reshape(-1) for p in per_sample]), n_a, c, size)


@pytest.mark.gpu
def test_a_batch_without_positives():
    head = _head(R.CASES['shipped'])
    rng = np.random.default_rng(4)
    maps = [rng.normal(-2.0, 1.5, (2, 18, R.H, R.W)).astype(np.float32), rng.normal(0, 0.3, (2, 42, R.H, R.W)).astype(np.float32),
            rng.normal(0, 1.0, (2, 12, R.H, R.W)).astype(np.float32)]
    empty = [torch.zeros((0, 7), device=DEV), torch.zeros((0, 7), device=DEV)]
    got = _gpu_losses(head, maps, empty, [torch.zeros(0, dtype=torch.long, device=DEV)] * 2)
    print('no positives:', {k: v for k, v in got.items() if k.startswith('loss')})
    assert got['loss_bbox'] == 0 and got['loss_dir'] == 0 and got['loss_cls'] > 0
    assert (got['d_bbox'] == 0).all() and (got['d_dir'] == 0).all() and np.isfinite(got['d_cls']).all() and (got['d_cls'] != 0).any()
    dense, _, n_pos, _ = R.batch_targets(_host_grid(head.anchor_generator.grid((R.H, R.W), DEV)), [np.zeros((0, 7), np.float32)] * 2,
                                         [np.zeros(0, np.int64)] * 2, R.CASES['shipped'], np.float64)
    want = R.loss_and_grads(*maps, dense, n_pos, R.CASES['shipped'])
    assert n_pos == 2
    _check_losses(got, want, {}, 'no positives')


@pytest.mark.gpu
def test_loss_reads_nothing_back(gold):
    cfg = R.CASES['shipped']
    head = _head(cfg)
    boxes, labels = _scene(gold, 'shipped')
    gts, lbs = [_t(b) for b in boxes], [_t(l) for l in labels]
    maps = [_t(gold[f'maps_6x3_{k}'].astype(np.float32)).requires_grad_(True) for k in ('cls', 'box', 'dir')]
    head.anchor_generator.grid((R.H, R.W), DEV)          # the tables are formed once per feature-map size
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = head.loss([maps[0]], [maps[1]], [maps[2]], gts, lbs, [None] * 3)
        (out['loss_cls'][0] + out['loss_bbox'][0] + out['loss_dir'][0]).backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert abs(out['loss_cls'][0].item() - float(gold['loss_shipped_f64_loss_cls'])) < 1e-4


def _check_candidates(got, want, what):
    boxes, scores, dirs, bev = [x.cpu().numpy() for x in got]
    _, r_boxes, r_scores, r_dirs, _ = want
    exact = [0, 1, 6]
    assert np.array_equal(boxes[:, exact].view(np.int32), r_boxes[:, exact].view(np.int32)), f'{what}: x, y, yaw bit for bit'
    d_exp = R.ulp_distance(boxes[:, 3:6], r_boxes[:, 3:6]).max()
    d_sig = R.ulp_distance(scores, r_scores).max()
    z_allowed = ULP_MATH * np.spacing(np.abs(r_boxes[:, 5])) / 2 + np.spacing(np.abs(r_boxes[:, 2])) + np.spacing(np.abs(boxes[:, 2]))
    z_err = (np.abs(boxes[:, 2].astype(np.float64) - r_boxes[:, 2]) / z_allowed).max()
    print(f'{what}: {len(boxes)} candidates, exp within {d_exp} ulp, sigmoid within {d_sig} ulp, z error / allowed {z_err:.2f}')
    assert d_exp <= ULP_MATH and d_sig <= ULP_MATH and z_err <= 1
    assert (scores[:, -1] == 0).all() and np.array_equal(dirs, r_dirs) and dirs.dtype == np.int64
    hw, hl = boxes[:, 3] / np.float32(2), boxes[:, 4] / np.float32(2)
    want_bev = np.stack([boxes[:, 0] - hw, boxes[:, 1] - hl, boxes[:, 0] + hw, boxes[:, 1] + hl, boxes[:, 6]], 1)
    assert np.array_equal(bev.view(np.int32), want_bev.astype(np.float32).view(np.int32)), f'{what}: the NMS rows'


def _box_error(got, want):
    """largest error of the final boxes over what the number formats allow: the sizes are within ULP_MATH ulp (exp), x, y and the
    yaw come from exact operations on equal inputs, z = zt * ha + za - hg / 2 carries the height's ULP_MATH ulp (of the larger of
    |z| and h) and two more roundings"""
    allowed = (ULP_MATH + 2) * np.spacing(np.maximum(np.abs(want), np.abs(want[:, 5:6])))
    return (np.abs(got.astype(np.float64) - want) / allowed).max() if len(want) else 0.0


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['shipped', 'smooth', 'ped_cyc'])
def test_decode_and_get_bboxes_equal_the_reference(gold, case):
    import sst_amd
    cfg = R.CASES[case]
    head = _head(cfg)
    n_a, c = head.num_anchors, cfg['num_classes']
    maps = [gold[f'maps_{n_a}x{c}_{k}'].astype(np.float32) for k in ('cls', 'box', 'dir')]
    dev = [_t(m) for m in maps]
    grid = head.anchor_generator.grid((R.H, R.W), DEV)
    host = _host_grid(grid)
    nms_pre = cfg['test_cfg']['nms_pre']
    assert (grid.num_anchors > nms_pre) == (case == 'smooth')          # both sides of `A > nms_pre`
    for s in range(3):
        want = R.candidates(host, maps[0][s], maps[1][s], maps[2][s], c, nms_pre)
        inds = _t(want[0]) if grid.num_anchors > nms_pre else None
        got = sst_amd.anchor_decode(dev[0][s], dev[1][s], dev[2][s], grid, c, inds)
        _check_candidates(got, want, f'{case} sample {s}')
    res = head.get_bboxes([dev[0]], [dev[1]], [dev[2]], [dict()] * 3)
    for s, (boxes, scores, labels) in enumerate(res):
        want_b, want_s, want_l = (gold[f'det_{case}_s{s}_{k}'] for k in ('bboxes', 'scores', 'labels'))
        assert labels.dtype == torch.long and np.array_equal(labels.cpu().numpy(), want_l), 'kept set, order and labels'
        d = R.ulp_distance(scores.cpu().numpy(), want_s).max()
        err = _box_error(boxes.cpu().numpy(), want_b)
        print(f'{case} sample {s}: {len(want_l)} boxes, scores within {d} ulp, box error / allowed {err:.2f}')
        assert d <= ULP_MATH and err <= 1


class _Boxes(object):
    def __init__(self, tensor, box_dim=7):
        self.tensor = tensor


@pytest.mark.gpu
def test_neck_and_head_end_to_end():
    """a 32 x 32 canvas: SECONDFPN -> forward_train / get_bboxes against the same modules run piecewise (torch convolutions, then
    the restatement on the maps copied to the host); backward reaches the three convolutions and the neck"""
    import sst_amd
    torch.manual_seed(0)
    rng = np.random.default_rng(8)
    gen = dict(R.generator_cfg(), ranges=[[-10.24, -10.24, z, 10.24, 10.24, z] for z in (-0.0345, -0.1188, 0.0)])
    cfg = dict(R.CASES['shipped'], anchor_generator=gen, test_cfg=dict(R.TEST_CFG, nms_pre=1000, score_thr=0.3))
    neck = sst_amd.build_neck(dict(type='SECONDFPN', norm_cfg=dict(type='naiveSyncBN2d', eps=1e-3, momentum=0.01),
                                   in_channels=[16], upsample_strides=[1], out_channels=[24])).to(DEV)
    head = _head(cfg, channels=24)
    with torch.no_grad():       # weights large enough that scores spread over the threshold
        for conv in (head.conv_cls, head.conv_reg, head.conv_dir_cls):
            conv.weight.normal_(0, 0.3)
        head.conv_cls.bias.fill_(-2.0)
    x = torch.randn(2, 16, 32, 32, device=DEV)
    samples = [_detector_like(rng, 10, -9.0, 9.0), _detector_like(rng, 6, -9.0, 9.0)]
    gts, lbs = [_Boxes(_t(b)) for b, _ in samples], [_t(l) for _, l in samples]
    losses = head.forward_train(neck([x]), gts, lbs, [dict()] * 2)
    total = losses['loss_cls'][0] + losses['loss_bbox'][0] + losses['loss_dir'][0]
    total.backward()
    for p in list(neck.parameters()) + [head.conv_cls.weight, head.conv_reg.weight, head.conv_dir_cls.weight, head.conv_cls.bias]:
        assert p.grad is not None and torch.isfinite(p.grad).all() and (p.grad != 0).any()
    with torch.no_grad():
        cls, box, dirs = head(neck([x]))
    maps = [m[0].cpu().numpy() for m in (cls, box, dirs)]
    grid = _host_grid(head.anchor_generator.grid((32, 32), DEV))
    dense64, _, n_pos, _ = R.batch_targets(grid, [b for b, _ in samples], [l for _, l in samples], cfg, np.float64)
    want = R.loss_and_grads(*maps, dense64, n_pos, cfg)
    got = {k: losses[k][0].item() for k in ('loss_cls', 'loss_bbox', 'loss_dir')}
    got.update(d_cls=None, d_bbox=None, d_dir=None)
    _check_losses(got, want, {}, 'end to end')
    neck.eval()
    with torch.no_grad():
        cls, box, dirs = head(neck([x]))
        res = head.get_bboxes(cls, box, dirs, [dict(box_type_3d=_Boxes)] * 2)
    maps = [m[0].cpu().numpy() for m in (cls, box, dirs)]
    for s, (boxes, scores, labels) in enumerate(res):
        assert isinstance(boxes, _Boxes)
        w_boxes, w_scores, w_labels = R.get_bboxes_single(grid, maps[0][s], maps[1][s], maps[2][s], cfg)
        assert 0 < len(w_labels) and np.array_equal(labels.cpu().numpy(), w_labels)
        err = _box_error(boxes.tensor.cpu().numpy(), w_boxes)
        print(f'end to end sample {s}: {len(w_labels)} boxes, box error / allowed {err:.2f}')
        assert R.ulp_distance(scores.cpu().numpy(), w_scores).max() <= ULP_MATH and err <= 1
