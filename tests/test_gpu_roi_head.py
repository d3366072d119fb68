"""The kernels of csrc/roi_head.hip and the heads of sst_amd/roi_head.py on the GPU against the reference's own results
(tests/golden/roi_head_train.npz) and the restatement of tests/roi_head_ref.py.  Rules: the IoU matrix bit for
bit equal to box_ops.boxes3d_overlaps_lidar under the class / sample mask; assignment, chosen sets, order, counts, labels and
reg_mask exactly; soft labels, targets, losses, gradients and decoded boxes within max(4 x the reference's own float32-vs-float64
gap, 1e-6) of the float64 restatement (losses: relative; vectors: of the largest element).  Every test prints what it achieved."""
import ast
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

import roi_head_ref as R
from test_roi_head_host import LOSS_CASES, gold_rows, gold_scene, loss_kwargs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EXACT = ('src', 'gt_index', 'labels', 'reg_mask', 'counts', 'assigned', 'argmax')


@pytest.fixture(scope='module')
def gold():
    return load_golden('roi_head_train.npz')


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def fused(scene, cfg, keys=None, generator=None):
    """sst_amd.roi_assign_sample on a scene of numpy arrays -> dict of numpy arrays"""
    import sst_amd
    props, plabels, gts, glabels = scene
    out = sst_amd.roi_assign_sample([dev(p) for p in props], [dev(l) for l in plabels], [dev(g) for g in gts],
                                    [dev(l) for l in glabels], keys=None if keys is None else dev(keys), generator=generator, **cfg)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in out.items()}


def gpu_overlap_fn(got, scene):
    """the restatement's IoU source: the kernel's own matrix (checked bit for bit against the box ops elsewhere), so that every
    decision and tie of the restatement is taken on the same values"""
    props, _ = R.with_fake_boxes(scene[0], scene[1])
    starts = np.cumsum([0] + [len(p) for p in props])
    table = {}
    for s, p in enumerate(props):
        table[len(table)] = (starts[s], len(p), len(scene[2][s]))
    calls = iter(range(len(props)))

    def fn(p, g, dtype):
        s = next(calls)
        while table[s][2] == 0:      # a sample without boxes asks for no matrix
            s = next(calls)
        p0, n, m = table[s]
        assert (n, m) == (len(p), len(g))
        return np.where(got['overlaps'][p0:p0 + n, :m] < 0, 0, got['overlaps'][p0:p0 + n, :m]).astype(dtype)
    return fn


def vector_error(got, ref):
    ref = np.asarray(ref, np.float64)
    scale = np.abs(ref).max() if ref.size else 0
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / scale) if scale else float(np.abs(got).max(initial=0))


def check_against_restatement(scene, cfg, keys, what):
    got = fused(scene, cfg, keys)
    r32 = R.assign_sample(*scene, cfg, keys, np.float32, gpu_overlap_fn(got, scene))
    r64 = R.assign_sample(*scene, cfg, keys, np.float64, gpu_overlap_fn(got, scene))
    for k in EXACT:
        assert np.array_equal(got[k], r32[k]), (what, k)
        assert np.array_equal(r32[k], r64[k]), (what, k, 'the scene decides on a rounding error')
    assert np.array_equal(got['rois'], r32['rois']) and np.array_equal(got['iou'], r32['iou']), what
    assert np.array_equal(got['max_overlaps'], r32['max_overlaps']), what
    worst = {}
    for k in ('soft_label', 'targets'):
        tol = max(4 * vector_error(r32[k], r64[k]), 1e-6)
        worst[k] = vector_error(got[k], r64[k])
        assert worst[k] <= tol, (what, k, worst[k], tol)
    print(f'{what}: counts {got["counts"].tolist()}, pools {r32["pool_sizes"]}; integers, rows and IoU equal; soft labels within '
          f'{worst["soft_label"]:.1e}, targets within {worst["targets"]:.1e} of float64')
    return got, r64


def test_iou_matrix_is_bit_equal_to_the_box_ops():
    import sst_amd
    tile = sst_amd.roi_head.roi_assign_gt_tile()
    scene = R.make_scene(11, [150, 1, 70, 0], [tile + 5, 3, 0, 7], cols=9, gt_cols=9)
    for class_mask in (True, False):
        cfg = R.with_cfg(class_mask=class_mask) if class_mask else R.with_cfg(class_mask=False, pos_iou_thr=0.45, neg_iou_thr=0.45,
                                                                              min_pos_iou=0.45)
        got = fused(scene, cfg, R.make_keys(0, scene[0]))
        props, plabels = R.with_fake_boxes(scene[0], scene[1])
        p0 = checked = 0
        for p, pl, g, gl in zip(props, plabels, scene[2], scene[3]):
            n, m = len(p), len(g)
            block = got['overlaps'][p0:p0 + n]
            assert (block[:, m:] == -1).all()
            if m:
                ref = sst_amd.box_ops.boxes3d_overlaps_lidar(dev(p[:, :7]), dev(g[:, :7])).cpu().numpy()
                mask = ((pl >= 0) & (pl < 3))[:, None] & ((gl >= 0) & (gl < 3))[None]
                if class_mask:
                    mask &= pl[:, None] == gl[None]
                assert np.array_equal(block[:, :m], np.where(mask, ref, np.float32(-1)))
                checked += int(mask.sum())
                mx = np.where(mask.any(1), np.where(mask, ref, -1).max(1), 0)
                assert np.array_equal(got['max_overlaps'][p0:p0 + n], mx.astype(np.float32))
            p0 += n
        print(f'class_mask={class_mask}: {checked} unmasked IoUs bit-equal to boxes3d_overlaps_lidar, '
              f'{int((got["overlaps"] > 0).sum())} of them positive')
        assert (got['overlaps'] > 0.3).sum() > 20


def sweep_cases():
    num, tile = R.WAYMO_CFG['num'], 64
    return {
        'props_small': ([0, 1, 63, 64], [5, 5, 5, 5]),
        'props_large': ([65, num, num + 1, 1500], [9, 9, 9, 30]),
        'props_workgroup_edges': ([255, 257, 511, 513], [6, 6, 12, 12]),     # the sampling kernel's 256 threads
        'boxes': ([90, 90, 90, 90, 90], [0, 1, tile - 1, tile, tile + 1]),
        'boxes_two_tiles': ([300, 40], [2 * tile + 1, 2 * tile]),
    }


@pytest.mark.parametrize('case', list(sweep_cases()))
def test_assignment_sampling_and_targets_at_every_size(case):
    import sst_amd
    assert sst_amd.roi_head.roi_assign_gt_tile() == 64 and sst_amd.roi_head.roi_assign_block() == 64
    prop_lens, gt_lens = sweep_cases()[case]
    scene = R.make_scene(len(case), prop_lens, gt_lens)
    check_against_restatement(scene, R.WAYMO_CFG, R.make_keys(5, scene[0]), case)


def test_the_single_assigner_form_and_nine_columns():
    scene = R.make_scene(21, [400, 30], [25, 4], cols=9, gt_cols=9)
    cfg = R.with_cfg(class_mask=False, pos_iou_thr=0.45, neg_iou_thr=0.3, min_pos_iou=0.2, num=128, neg_piece_fractions=[0.5, 0.3, 0.2],
                     neg_iou_piece_thrs=[0.3, 0.1, 0.02], cls_pos_thr=0.75, cls_neg_thr=0.25)
    got, _ = check_against_restatement(scene, cfg, R.make_keys(2, scene[0]), 'single assigner, 9 columns, three pieces')
    assert (got['assigned'] == -2).any(), 'the scene has ignored proposals (neg_iou_thr < pos_iou_thr)'


def test_runs_are_bit_reproducible_and_the_seed_only_changes_the_choice():
    scene = R.make_scene(4, [900, 500], [20, 12])
    keys = R.make_keys(9, scene[0])
    a, b = fused(scene, R.WAYMO_CFG, keys), fused(scene, R.WAYMO_CFG, keys)
    for k in R.ROW_KEYS + ('counts', 'overlaps', 'max_overlaps', 'argmax', 'assigned'):
        assert a[k].tobytes() == b[k].tobytes(), k
    runs = []
    for seed in (1, 1, 2):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(seed)
        runs.append(fused(scene, R.WAYMO_CFG, generator=gen))
    assert runs[0]['src'].tobytes() == runs[1]['src'].tobytes() and runs[0]['targets'].tobytes() == runs[1]['targets'].tobytes()
    assert np.array_equal(runs[0]['counts'], runs[2]['counts']) and np.array_equal(runs[0]['assigned'], runs[2]['assigned'])
    assert not np.array_equal(runs[0]['src'], runs[2]['src'])
    # the pools are the same sets: the rows of a piece drawn under either seed lie in the same IoU band
    print(f'two runs bit-equal; seeds 1 and 2 share counts {runs[0]["counts"].tolist()} and differ in '
          f'{int((runs[0]["src"] != runs[2]["src"]).sum())} of {runs[0]["src"].size} rows')


def gpu_losses(cls_score, bbox_pred, nonempty, rows, gts, upstream=(1.0, 1.0, 1.0), **kw):
    import sst_amd
    z, bp = dev(cls_score).requires_grad_(True), dev(bbox_pred).requires_grad_(True)
    out = sst_amd.roi_loss(z, bp, dev(nonempty), dev(rows['rois']), dev(rows['soft_label'], torch.float32), dev(rows['reg_mask']),
                           dev(rows['targets'], torch.float32), dev(rows['gt_index']), dev(rows['labels']), dev(gts), **kw)
    loss_cls, loss_bbox, loss_corner, num, counts = out
    (upstream[0] * loss_cls + upstream[1] * loss_bbox + upstream[2] * loss_corner).backward()
    torch.cuda.synchronize()
    return dict(loss_cls=float(loss_cls.detach()), loss_bbox=float(loss_bbox.detach()), loss_corner=float(loss_corner.detach()), num_pos=int(num[0]),
                num_neg=int(num[1]), corner_rows=int(counts[1]), d_cls=z.grad.cpu().numpy(), d_bbox=bp.grad.cpu().numpy())


def compare_losses(got, r64, r32, what, noise=None):
    for k in ('num_pos', 'num_neg', 'corner_rows'):
        assert got[k] == r64[k], (what, k, got[k], r64[k])
    report = []
    for k in ('loss_cls', 'loss_bbox', 'loss_corner'):
        gap = float(noise[k]) if noise is not None else abs(r32[k] - r64[k]) / abs(r64[k]) if r64[k] else abs(r32[k])
        tol = max(4 * gap, 1e-6)
        err = abs(got[k] - r64[k]) / abs(r64[k]) if r64[k] else abs(got[k])
        report.append(f'{k} {got[k]:.8g} vs {r64[k]:.8g} ({err:.1e} <= {tol:.1e})')
        assert err <= tol, (what, k, got[k], r64[k], err, tol)
        if r64[k] == 0:
            assert got[k] == 0
    for k in ('d_cls', 'd_bbox'):
        tol = max(4 * (float(noise[k]) if noise is not None else vector_error(r32[k], r64[k])), 1e-6)
        err = vector_error(got[k], r64[k])
        report.append(f'{k} {err:.1e} <= {tol:.1e}')
        assert np.array_equal(got[k] != 0, r64[k] != 0) or err <= tol, (what, k)
        assert err <= tol, (what, k, err, tol)
    print(f'{what}: pos {got["num_pos"]}, corner rows {got["corner_rows"]}; ' + '; '.join(report))


@pytest.fixture(scope='module')
def loss_scene():
    scene = R.make_scene(8, [700, 300, 1], [30, 10, 2])
    rows = R.compact(R.assign_sample(*scene, R.WAYMO_CFG, R.make_keys(3, scene[0]), np.float32))
    rows['soft_label'], rows['targets'] = rows['soft_label'].astype(np.float32), rows['targets'].astype(np.float32)
    z, bp, nonempty = R.make_predictions(1, len(rows['src']))
    return rows, np.concatenate(scene[2]), z, bp, nonempty


@pytest.mark.parametrize('beta', [0.0, 1.0 / 9.0])
@pytest.mark.parametrize('code_weight', [None, [1.0, 1.0, 2.0, 0.5, 0.5, 0.25, 3.0]])
@pytest.mark.parametrize('corner', ['off', 'car', 'all'])
def test_losses_and_gradients(loss_scene, beta, code_weight, corner):
    rows, gts, z, bp, nonempty = loss_scene
    kw = dict(loss_weights=(1.0, 2.0, 1.5), beta=beta, code_weight=code_weight, with_corner=corner != 'off',
              car_index=0 if corner == 'car' else -1, upstream=(0.7, 1.3, -2.0))
    r64, r32 = R.losses(z, bp, nonempty, rows, gts, dtype=torch.float64, **kw), R.losses(z, bp, nonempty, rows, gts, dtype=torch.float32, **kw)
    got = gpu_losses(z, bp, nonempty, rows, gts, upstream=kw['upstream'], loss_weights=kw['loss_weights'], smooth_l1_beta=beta,
                     code_weight=code_weight, with_corner_loss=kw['with_corner'], car_index=kw['car_index'])
    assert r64['num_pos'] > 20 and (corner == 'off' or r64['corner_rows'] > 5)
    compare_losses(got, r64, r32, f'beta {beta:.3f}, code_weight {code_weight is not None}, corner {corner}')


@pytest.mark.parametrize('case', ['all_empty', 'no_positive', 'no_car', 'one_row'])
def test_losses_at_the_degenerate_ends(loss_scene, case):
    rows, gts, z, bp, nonempty = loss_scene
    rows = dict(rows)
    if case == 'all_empty':
        nonempty = np.zeros_like(nonempty)
    elif case == 'no_positive':
        nonempty = nonempty & (rows['reg_mask'] == 0)
    elif case == 'no_car':
        nonempty = nonempty & ~((rows['reg_mask'] == 1) & (rows['labels'] == 0))
    else:
        first = int(np.nonzero((rows['reg_mask'] == 1) & (rows['labels'] == 0))[0][0])
        rows = {k: (v[first:first + 1] if k in R.ROW_KEYS else v) for k, v in rows.items()}
        z, bp, nonempty = z[first:first + 1], bp[first:first + 1], np.ones(1, bool)
    kw = dict(loss_weights=(1.0, 2.0, 1.0), with_corner=True, car_index=0)
    r64, r32 = R.losses(z, bp, nonempty, rows, gts, dtype=torch.float64, **kw), R.losses(z, bp, nonempty, rows, gts, dtype=torch.float32, **kw)
    got = gpu_losses(z, bp, nonempty, rows, gts, loss_weights=kw['loss_weights'], with_corner_loss=True, car_index=0)
    if case in ('all_empty', 'no_positive'):
        assert got['loss_bbox'] == 0 and got['loss_corner'] == 0 and got['num_pos'] == 0 and not got['d_bbox'].any()
    if case == 'all_empty':
        assert got['loss_cls'] == 0 and not got['d_cls'].any()
    if case == 'no_car':
        assert got['loss_corner'] == 0 and got['corner_rows'] == 0 and got['loss_bbox'] > 0
    compare_losses(got, r64, r32, case)


def test_decode_equals_the_restatement(loss_scene):
    import sst_amd
    rows, _, z, bp, _ = loss_scene
    for cols in (7, 9):
        rois = rows['rois'] if cols == 7 else np.concatenate([rows['rois'], np.random.default_rng(0).normal(0, 2, (len(z), 2)).astype(np.float32)], 1)
        boxes, scores, bev = (t.cpu().numpy() for t in sst_amd.roi_decode(dev(rois), dev(bp), dev(z)))
        r64, r32 = R.decode(rois, bp, z, torch.float64), R.decode(rois, bp, z, torch.float32)
        assert boxes.shape == (len(z), cols) and np.array_equal(boxes[:, 7:], rois[:, 8:])
        errs = []
        for got, a, b in zip((boxes, scores, bev), r64, r32):
            tol = max(4 * vector_error(b, a), 1e-6)
            errs.append(vector_error(got, a))
            assert errs[-1] <= tol
        print(f'{cols} columns: boxes within {errs[0]:.1e}, scores {errs[1]:.1e}, NMS rows {errs[2]:.1e} of float64')


# ---- against the reference's own results ---------------------------------------------------------------------------

def test_assignment_sampling_and_targets_equal_the_reference(gold):
    scene, keys = gold_scene(gold)
    got = fused(scene, R.WAYMO_CFG, keys)
    ref = gold_rows(gold)
    rows = R.compact(got)
    assert np.array_equal(got['counts'], gold['counts'])
    for k in ('src', 'gt_index', 'labels', 'reg_mask'):
        assert np.array_equal(rows[k], ref[k]), k
    assert np.array_equal(got['assigned'], gold['assigned'])
    assert np.array_equal(rows['rois'], ref['rois'])
    report = {}
    for k, ref_v in (('iou', ref['iou_f64']), ('soft_label', ref['soft_label_f64']), ('targets', ref['targets_f64'])):
        tol = max(4 * float(gold['noise_' + k]), 1e-6)
        # the IoU itself is held to the bar of the box ops (tests/box_ops_ref.py: F32_IOU_NOISE, absolute)
        err = float(np.abs(rows[k] - ref_v).max()) if k == 'iou' else vector_error(rows[k], ref_v)
        tol = max(tol, 1e-5) if k in ('iou', 'soft_label') else tol
        report[k] = (err, tol)
        assert err <= tol, (k, err, tol)
    print(f'reference scene: counts {got["counts"].tolist()}, every integer, set and order equal; ' +
          ', '.join(f'{k} within {e:.1e} (allowed {t:.1e})' for k, (e, t) in report.items()))
    check_against_restatement(scene, R.WAYMO_CFG, keys, 'reference scene vs restatement')


@pytest.mark.parametrize('case', list(LOSS_CASES))
def test_losses_and_gradients_equal_the_reference(gold, case):
    ref = gold_rows(gold)
    rows = dict(rois=ref['rois'], soft_label=ref['soft_label_f32'], reg_mask=ref['reg_mask'], targets=ref['targets_f32'],
                gt_index=ref['gt_index'], labels=ref['labels'])
    kw = loss_kwargs(case)
    z, bp, nonempty = gold['cls_score'].astype(np.float32), gold['bbox_pred'].astype(np.float32), gold[f'{case}_nonempty']
    got = gpu_losses(z, bp, nonempty, rows, gold['gts'], loss_weights=kw['loss_weights'], smooth_l1_beta=kw['beta'],
                     code_weight=kw['code_weight'], with_corner_loss=kw['with_corner'], car_index=kw['car_index'])
    r64 = {k: gold[f'{case}_f64_{k}'] for k in ('loss_cls', 'loss_bbox', 'loss_corner', 'd_cls', 'd_bbox')}
    r64 = {k: (float(v) if v.ndim == 0 else v) for k, v in r64.items()}
    r64.update(num_pos=int(gold[f'{case}_num_pos']), num_neg=int(gold[f'{case}_num_neg']), corner_rows=int(gold[f'{case}_corner_rows']))
    noise = {k: gold[f'noise_{case}_{k}'] for k in ('loss_cls', 'loss_bbox', 'loss_corner', 'd_cls', 'd_bbox')}
    compare_losses(got, r64, None, case + ' vs reference', noise)


def test_decode_and_get_bboxes_equal_the_reference(gold):
    import sst_amd
    head = sst_amd.build_head(dict(_small_head(), test_cfg=dict(use_rotate_nms=True, nms_pre=-1, nms_thr=0.25, score_thr=0.1,
                                                                 min_bbox_size=0, max_num=500))).to(DEV)
    rois, z, bp = gold['test_rois'], gold['test_cls_score'].astype(np.float32), gold['test_bbox_pred'].astype(np.float32)
    boxes = head.decode_from_rois(dev(rois), dev(bp)).cpu().numpy()
    tol = max(4 * float(gold['noise_test_boxes']), 1e-6)
    err = vector_error(boxes, gold['test_boxes_f64'])
    assert err <= tol
    out = head.get_bboxes(dev(rois), dev(z), dev(bp), dev(gold['test_valid']), [dev(gold['test_labels'])], [dev(gold['test_scores'])],
                          [dict()])
    sel_boxes, sel_scores, sel_labels = (t.cpu().numpy() for t in out[0])
    keep = gold['test_selected']
    valid = np.nonzero(gold['test_valid'])[0]
    assert len(sel_scores) == len(keep) and np.array_equal(sel_labels, gold['test_labels'][valid][keep])
    assert np.array_equal(sel_boxes, boxes[valid][keep])
    sig = 1 / (1 + np.exp(-z.astype(np.float64).reshape(-1)))
    assert np.abs(sel_scores - sig[valid][keep]).max() <= 1e-6
    print(f'decoded boxes within {err:.1e} (allowed {tol:.1e}); {len(keep)} of {len(valid)} boxes kept, the reference\'s keep list in '
          f'its order')


# ---- end to end ------------------------------------------------------------------------------------------------------

def _small_head():
    return dict(type='FullySparseBboxHead', num_classes=3, num_blocks=2, in_channels=[16 + 3 + 13, 16 + 3 + 13],
                feat_channels=[[16, 16], [16, 16]], rel_mlp_hidden_dims=[[8], [8]], rel_mlp_in_channels=[13, 13], reg_mlp=[32],
                cls_mlp=[32], with_corner_loss=True, norm_cfg=dict(type='LN', eps=1e-3), unique_once=True,
                loss_bbox=dict(type='L1Loss', reduction='mean', loss_weight=2.0),
                loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, reduction='mean', loss_weight=1.0))


def _frame(seed, n_samples, pts_per_sample, n_objects, xyz_dim, feat_dim):
    """points (xyz and the further point columns the head is fed, as intensity and elongation) on a few box-shaped clusters per
    sample, proposals jittered about the boxes, the boxes as ground truth"""
    rng = np.random.default_rng(seed)
    xyz, bidx, proposals, gts, glabels = [], [], [], [], []
    for s in range(n_samples):
        g = R.random_boxes(rng, n_objects, 7, 30.0)
        g[:, 6] = rng.uniform(-np.pi, np.pi, n_objects)
        gl = rng.integers(0, 3, n_objects)
        of = rng.integers(0, n_objects, pts_per_sample)
        local = rng.uniform(-0.5, 0.5, (pts_per_sample, 3)) * g[of, 3:6]
        c, sn = np.cos(g[of, 6]), np.sin(g[of, 6])
        pts = np.stack([local[:, 0] * c + local[:, 1] * sn + g[of, 0], -local[:, 0] * sn + local[:, 1] * c + g[of, 1],
                        local[:, 2] + g[of, 2] + g[of, 5] / 2], 1)
        k = 4 * n_objects
        src = rng.integers(0, n_objects, k)
        p = g[src] + (rng.normal(0, 1, (k, 7)) * np.array([0.3, 0.3, 0.1, 0.1, 0.2, 0.1, 0.1])).astype(np.float32)
        far = R.random_boxes(rng, n_objects, 7, 30.0)
        proposals.append((dev(np.concatenate([p, far]).astype(np.float32)), dev(rng.random(k + n_objects).astype(np.float32)),
                          dev(np.concatenate([gl[src], rng.integers(0, 3, n_objects)]).astype(np.int64))))
        xyz.append(pts.astype(np.float32)), bidx.append(np.full(pts_per_sample, s, np.int64))
        gts.append(dev(g)), glabels.append(dev(gl.astype(np.int64)))
    xyz = np.concatenate(xyz)
    xyz = np.concatenate([xyz, rng.random((len(xyz), xyz_dim - 3)).astype(np.float32)], 1)
    feats = rng.normal(0, 1, (len(xyz), feat_dim)).astype(np.float32)
    return dev(xyz), dev(feats), dev(np.concatenate(bidx)), proposals, gts, glabels


def test_the_network_aligns_its_rows_with_the_rois():
    """5 RoIs, RoI 1 and RoI 4 without a point, two points of no RoI (-1)"""
    import sst_amd
    torch.manual_seed(0)
    head = sst_amd.build_head(dict(type='FullySparseBboxHead', num_classes=3, num_blocks=2, in_channels=[8 + 3 + 13, 16 + 3 + 13],
                                   feat_channels=[[16, 16], [16, 16]], rel_mlp_hidden_dims=[[8], [8]], rel_mlp_in_channels=[13, 13],
                                   reg_mlp=[32], cls_mlp=[32], norm_cfg=dict(type='LN', eps=1e-3), unique_once=True,
                                   loss_bbox=dict(type='L1Loss', loss_weight=2.0),
                                   loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, reduction='mean')))
    head = head.to(DEV).eval()
    roi_inds = torch.tensor([-1, 0, 0, 2, 2, 2, 3, -1, 0]).sort()[0].to(DEV)
    n = len(roi_inds)
    info = dict(local_xyz=torch.randn(n, 3).to(DEV), boundary_offset=torch.randn(n, 6).to(DEV), is_in_margin=torch.zeros(n).to(DEV))
    rois = torch.cat([torch.zeros(5, 1), torch.randn(5, 3), torch.rand(5, 3) + 1, torch.randn(5, 1)], 1).to(DEV)
    cls_score, bbox_pred, nonempty = head(torch.randn(n, 3).to(DEV), torch.randn(n, 8).to(DEV), info, roi_inds, rois)
    assert nonempty.tolist() == [True, False, True, True, False]
    assert tuple(cls_score.shape) == (5, 1) and tuple(bbox_pred.shape) == (5, 7)
    assert not cls_score[1].any() and not bbox_pred[4].any() and bbox_pred[0].any() and cls_score[3].any()
    # no RoI has a point: zeros that still reach the parameters
    cls_score, bbox_pred, nonempty = head(torch.randn(2, 3).to(DEV), torch.randn(2, 8).to(DEV), {k: v[:2] for k, v in info.items()},
                                          torch.tensor([-1, -1]).to(DEV), rois)
    assert not nonempty.any() and not cls_score.any() and cls_score.requires_grad


@pytest.mark.parametrize('name', ['fsd/fsd_waymoD1_1x', 'fsdv2/fsdv2_waymo_1x'])
def test_forward_train_and_backward_of_the_shipped_heads(name):
    import sst_amd
    model = ast.literal_eval(open(os.path.join(GOLDEN, 'configs', name + '.model.py')).read())
    det = sst_amd.build_detector(model)
    torch.manual_seed(0)
    head = sst_amd.build_head(dict(det.unbuilt['roi_head'], train_cfg=det.train_cfg['rcnn'], test_cfg=det.test_cfg['rcnn'])).to(DEV)
    head.train()
    bh = det.unbuilt['roi_head']['bbox_head']
    # a block's input: the point columns (xyz, intensity, ...), the features, the 13 geometric columns
    xyz_dim = bh['in_channels'][1] - bh['feat_channels'][0][-1] - 13
    xyz, feats, bidx, proposals, gts, glabels = _frame(5, 2, 2000, 12, xyz_dim, bh['in_channels'][0] - xyz_dim - 13)
    feats.requires_grad_(True)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    losses = head.forward_train(xyz, feats, bidx, [dict(), dict()], proposals, gts, glabels, generator=gen)
    assert set(losses) == {'loss_rcnn_cls', 'loss_rcnn_bbox', 'loss_rcnn_corner', 'num_pos_rois', 'num_neg_rois'}
    total = losses['loss_rcnn_cls'] + losses['loss_rcnn_bbox'] + losses['loss_rcnn_corner']
    total.backward()
    torch.cuda.synchronize()
    values = {k: float(v) for k, v in losses.items()}
    assert all(np.isfinite(v) for v in values.values()) and values['num_pos_rois'] > 10 and values['loss_rcnn_bbox'] > 0
    missing = [k for k, p in head.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not missing, missing
    assert feats.grad is not None and torch.isfinite(feats.grad).all() and feats.grad.abs().sum() > 0
    head.eval()
    out = head.simple_test(xyz[bidx == 0], feats.detach()[bidx == 0], bidx[bidx == 0], [dict()], proposals[:1])
    assert len(out) == 1 and out[0][0].size(1) == 7 and out[0][0].size(0) == out[0][1].size(0) == out[0][2].size(0)
    print(f'{name}: {values}; every one of {sum(1 for _ in head.parameters())} parameters has a finite gradient; simple_test kept '
          f'{out[0][0].size(0)} boxes')
