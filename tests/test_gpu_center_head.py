"""CenterHead's targets, losses and decoding on the GPU (csrc/center_head.hip) against the reference's golden
(tests/golden/center_head_train.npz) and the restatement of tests/center_head_ref.py.

Targets: ind, mask and the cells of the heatmap equal to 0 or to 1 exactly; every other heatmap cell within 1 float32 ulp (the
fp64 exp of the device and of numpy may round differently at a tie of the final rounding only); anno_box columns 0-2 and 8-9
bit for bit; columns 3-7 (log, sin, cos) within ULP_MATH.  Decoding: x, y, z and the velocities bit for bit, exp / atan2 within
ULP_MATH, keep sets exactly.

ULP_MATH = 2: the published HIP math API table of the ROCm documentation lists logf, sinf, cosf, expf and atan2f at a maximum
error of 1 ulp on the device; torch's CPU functions are SLEEF's 1.0-ulp routines (or the C library's, correctly rounded to within 1 ulp); both
sides are at most 1 ulp from the true value, hence at most 2 ulp from each other.

Losses (float64 autograd of the restatement on the same float32 inputs): relative error of each loss scalar and
max |err| / max |grad| of each gradient tensor <= max(4 * noise, 1e-6), noise = the reference's own float32-vs-float64 gap
stored in the golden; cases without a golden use the floor alone.  Every case prints its errors before it asserts (pytest -s)."""
import ast
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

import center_head_ref as R

DEV = 'cuda:0'
ULP_MATH = 2
HEADS = ('reg', 'height', 'dim', 'rot', 'vel')


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


@pytest.fixture(scope='module')
def gold():
    return load_golden('center_head_train.npz')


def _scene(gold, case):
    cols = R.CASES[case][3]
    return [gold[f'boxes{s}'][:, :cols] for s in range(3)], [gold[f'labels{s}'] for s in range(3)]


_RESTATED = {}


def _restated(gold, case):
    """the restated targets of a golden case, computed once and left unchanged"""
    if case not in _RESTATED:
        cfg, tasks, norm_bbox, _ = R.CASES[case]
        boxes, labels = _scene(gold, case)
        _RESTATED[case] = R.targets(boxes, labels, tasks, cfg, norm_bbox)
    return _RESTATED[case]


def _gpu_targets(boxes, labels, tasks, cfg, norm_bbox):
    import sst_amd
    out = sst_amd.center_targets([_t(b) for b in boxes], [_t(l) for l in labels], tasks, cfg, norm_bbox)
    return [[x.cpu().numpy() for x in lst] for lst in out]


def _check_targets(got, want_exact, want_heatmap, n_tasks, what):
    """got / want_exact: (heatmaps, annos, inds, masks); want_heatmap: the heatmaps the 0 / 1 pattern and the 1-ulp rule go by"""
    for t in range(n_tasks):
        hm, anno, ind, mask = (got[k][t] for k in range(4))
        r_hm, r_anno, r_ind, r_mask = (want_exact[k][t] for k in range(4))
        assert ind.dtype == np.int64 and mask.dtype == np.uint8 and hm.dtype == anno.dtype == np.float32
        assert np.array_equal(ind, r_ind) and np.array_equal(mask, r_mask), what
        for ref_hm in (r_hm, want_heatmap[t]):
            assert np.array_equal(hm == 1, ref_hm == 1) and np.array_equal(hm == 0, ref_hm == 0), what
            d = R.ulp_distance(hm, ref_hm).max()
            print(f'{what} task {t}: heatmap max ulp distance {d}, cells > 0: {(hm > 0).sum()}, peaks: {(hm == 1).sum()}')
            assert d <= 1
        assert np.array_equal(anno[..., [0, 1, 2, 8, 9]], r_anno[..., [0, 1, 2, 8, 9]]), what
        d = R.ulp_distance(anno[..., 3:8], r_anno[..., 3:8]).max()
        print(f'{what} task {t}: anno_box log / sin / cos max ulp distance {d}')
        assert d <= ULP_MATH


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(R.CASES))
def test_targets_equal_the_reference_and_the_restatement(gold, case):
    cfg, tasks, norm_bbox, _ = R.CASES[case]
    boxes, labels = _scene(gold, case)
    got = _gpu_targets(boxes, labels, tasks, cfg, norm_bbox)
    golden = [[gold[f'tgt_{case}_t{t}_{k}'] for t in range(len(tasks))] for k in ('heatmap', 'anno', 'ind', 'mask')]
    assert np.array_equal(golden[2][0], _restated(gold, case)[2][0])
    _check_targets(got, _restated(gold, case), golden[0], len(tasks), case)
    # against the golden's own anno_box too: its transcendental columns are torch's CPU functions on single boxes
    for t in range(len(tasks)):
        assert R.ulp_distance(got[1][t], golden[1][t]).max() <= ULP_MATH


def _shipped_cfg():
    path = os.path.join(GOLDEN, 'configs', 'sst_refactor', 'sst_waymoD5_1x_3class_centerhead.model.py')
    return ast.literal_eval(open(path).read())


def _launch_scene():
    """the shipped 468 x 468 map, two samples of 300 boxes: several workgroups per sample, 3 classes, borders, labels of -1"""
    rng = np.random.default_rng(5)
    boxes, labels = [], []
    for s in range(2):
        n = 300
        b = np.zeros((n, 9), np.float32)
        b[:, :2] = rng.uniform(-76.0, 76.0, (n, 2))            # some centres beyond the range on every side
        b[:, 2] = rng.uniform(-1.5, 0.5, n)
        kind = rng.integers(0, 3, n)
        b[:, 3:6] = np.float32([[2.0, 4.6, 1.6], [0.8, 0.9, 1.7], [2.9, 11.0, 3.4]])[kind] * rng.uniform(0.8, 1.25, (n, 3))
        b[:, 6] = rng.uniform(-np.pi, np.pi, n)
        b[:, 7:9] = rng.normal(0, 3.0, (n, 2))
        lab = kind.astype(np.int64)
        lab[rng.random(n) < 0.05] = -1
        boxes.append(b)
        labels.append(lab)
    return boxes, labels


@pytest.mark.gpu
def test_targets_at_the_launch_size_and_twice_the_same():
    import sst_amd
    model = _shipped_cfg()
    cfg, tasks = model['train_cfg'], model['bbox_head']['tasks']
    boxes, labels = _launch_scene()
    assert len(boxes[0]) > 4 * sst_amd.center_head.center_targets_box_tile()
    want = R.targets(boxes, labels, tasks, cfg, True)
    got = _gpu_targets(boxes, labels, tasks, cfg, True)
    assert got[0][0].shape == (2, 3, 468, 468) and got[2][0].shape == (2, 500)
    n_task = [(l >= 0).sum() for l in labels]
    assert all(0 < want[3][0][s].sum() < n_task[s] < 300 for s in range(2))       # some centres lie outside the map
    _check_targets(got, want, want[0], 1, 'launch size')
    again = _gpu_targets(boxes, labels, tasks, cfg, True)
    for a, b in zip(got, again):
        assert a[0].tobytes() == b[0].tobytes()


# ---- losses --------------------------------------------------------------------------------------------------------

def _loss_inputs(gold, case, t):
    tasks = R.CASES[case][1]
    at = sum(len(x['class_names']) for x in tasks[:t])
    c = len(tasks[t]['class_names'])
    logits = np.ascontiguousarray(gold['logits'][:, at:at + c])
    heads = R.split_heads(gold['head_maps'].astype(np.float32))
    return logits, heads


def _run_loss(logits, heads, tgt, code_weights, w_cls, w_bbox):
    """-> (loss_heatmap, loss_bbox, d_logits, [d_head], counts) as numpy, from one forward and one backward on the GPU"""
    import sst_amd
    lg = _t(logits).requires_grad_(True)
    hs = [None if h is None else _t(h).requires_grad_(True) for h in heads]
    hs += [None] * (5 - len(hs))
    before = lg.detach().clone()
    l_hm, l_box, counts = sst_amd.center_loss(lg, *hs, *[_t(x) for x in tgt], code_weights, w_cls, w_bbox)
    assert torch.equal(lg.detach(), before), 'the logits were modified'
    (l_hm * 1.5 + l_box * 0.5).backward()
    return (l_hm.item(), l_box.item(), lg.grad.cpu().numpy() / 1.5,
            [h.grad.cpu().numpy() / 0.5 for h in hs if h is not None], counts.cpu().numpy())


def _compare_losses(got, ref, noise, what):
    l_hm, l_box, d_logits, d_heads, _ = got
    failures = []
    for name, g, r in (('loss_heatmap', l_hm, float(ref['loss_heatmap'])), ('loss_bbox', l_box, float(ref['loss_bbox']))):
        err = abs(g - r) / max(abs(r), 1e-30) if r != 0 else abs(g)
        tol = max(4 * noise.get(name, 0.0), 1e-6)
        print(f'{what} {name}: {g!r} vs {r!r}, relative error {err:.3e} (tolerance {tol:.3e})')
        if not err <= tol:
            failures.append(name)
    tensors = [('d_logits', d_logits, ref['d_logits'], noise.get('d_logits', 0.0))]
    tensors += [(f'd_{HEADS[i]}', d_heads[i], ref['d_heads'][i], noise.get('d_heads', 0.0)) for i in range(len(d_heads))]
    for name, g, r, nz in tensors:
        scale = np.abs(r).max()
        err = np.abs(g.astype(np.float64) - r).max() / scale if scale > 0 else np.abs(g).max()
        tol = max(4 * nz, 1e-6)
        print(f'{what} {name}: max |err| / max |grad| {err:.3e} (tolerance {tol:.3e}), max |grad| {scale:.3e}')
        if not err <= tol:
            failures.append(name)
        if name != 'd_logits':
            assert not g[r == 0].any(), f'{what} {name}: a cell no kept slot names received a gradient'
    assert not failures, f'{what}: {failures}'


@pytest.mark.gpu
@pytest.mark.parametrize('case,t', [('shipped', 0), ('two_tasks', 0), ('two_tasks', 1)])
def test_losses_and_gradients_against_float64(gold, case, t):
    cfg = R.CASES[case][0]
    logits, heads = _loss_inputs(gold, case, t)
    tgt = [gold[f'tgt_{case}_t{t}_{k}'] for k in ('heatmap', 'anno', 'ind', 'mask')]
    ref = R.losses_and_grads(logits, heads, *tgt, cfg['code_weights'], R.W_CLS, R.W_BBOX)
    noise = {k: float(gold[f'noise_{case}_t{t}_{k}']) for k in ('loss_heatmap', 'loss_bbox', 'd_logits', 'd_heads')}
    got = _run_loss(logits, heads, tgt, cfg['code_weights'], R.W_CLS, R.W_BBOX)
    mask = tgt[3].astype(bool)
    assert got[4].tolist() == [int((tgt[0] == 1).sum()), int(mask.sum())]
    if case == 'shipped':
        # two kept slots of sample 0 name one cell: their gradients add
        cells, n = np.unique(tgt[2][0][mask[0]], return_counts=True)
        shared = cells[n > 1]
        assert len(shared) >= 2
        y, x = divmod(int(shared[0]), R.W)
        k = R.W_BBOX / (np.float32(mask.sum()) + np.float32(1e-4))
        assert set(np.round(np.abs(ref['d_heads'][0][0, :, y, x]) / k).astype(int)) <= {0, 2}
        assert not mask[1].any()                                   # and one sample has no boxes at all
    assert (np.abs(logits) > 9.3).any() and (got[2][np.abs(logits) > 9.3] == 0).all()    # zero where the clamp is active
    _compare_losses(got, ref, noise, f'{case} task {t}')
    again = _run_loss(logits, heads, tgt, cfg['code_weights'], R.W_CLS, R.W_BBOX)
    assert got[0] == again[0] and got[1] == again[1] and got[2].tobytes() == again[2].tobytes()
    for a, b in zip(got[3], again[3]):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_losses_without_a_single_box_and_without_the_velocity_head(gold):
    """num_pos = 0 and sum(mask) = 0: both losses finite, the box gradients exactly zero; four heads, eight code columns"""
    cfg, tasks, norm_bbox, _ = R.CASES['shipped']
    empty = [np.zeros((0, 7), np.float32)] * 3, [np.zeros(0, np.int64)] * 3
    tgt = [x[0] for x in _gpu_targets(*empty, tasks, cfg, norm_bbox)]
    assert not tgt[0].any() and not tgt[3].any() and not tgt[2].any() and not tgt[1].any()
    logits, heads = _loss_inputs(gold, 'shipped', 0)
    heads = heads[:4]
    ref = R.losses_and_grads(logits, heads, *tgt, cfg['code_weights'], R.W_CLS, R.W_BBOX)
    got = _run_loss(logits, heads, tgt, cfg['code_weights'], R.W_CLS, R.W_BBOX)
    assert np.isfinite(got[0]) and got[1] == 0.0 and got[4].tolist() == [0, 0]
    assert all(not g.any() for g in got[3]) and len(got[3]) == 4
    _compare_losses(got, ref, {}, 'no boxes')
    # the kept slots of the golden case on four heads
    tgt = [gold[f'tgt_shipped_t0_{k}'] for k in ('heatmap', 'anno', 'ind', 'mask')]
    ref = R.losses_and_grads(logits, heads, *tgt, cfg['code_weights'], R.W_CLS, R.W_BBOX)
    _compare_losses(_run_loss(logits, heads, tgt, cfg['code_weights'], R.W_CLS, R.W_BBOX), ref, {}, 'four heads')


@pytest.mark.gpu
def test_losses_at_the_launch_size():
    """the shipped head's sizes: 2 x 3 x 468 x 468 logits in 321 partial records, 500 slots per sample"""
    model = _shipped_cfg()
    cfg, tasks = model['train_cfg'], model['bbox_head']['tasks']
    boxes, labels = _launch_scene()
    tgt = [x[0] for x in _gpu_targets(boxes, labels, tasks, cfg, True)]
    rng = np.random.default_rng(6)
    logits = rng.normal(-2.0, 2.5, (2, 3, 468, 468)).astype(np.float32)
    heads = R.split_heads(rng.normal(0, 1.0, (2, 10, 468, 468)).astype(np.float32))
    ref = R.losses_and_grads(logits, heads, *tgt, cfg['code_weights'], 1.0, 2.0)
    got = _run_loss(logits, heads, tgt, cfg['code_weights'], 1.0, 2.0)
    _compare_losses(got, ref, {}, 'launch size')


# ---- decoding ------------------------------------------------------------------------------------------------------

def _decode_inputs(gold, case):
    with_vel = R.DECODE_CASES[case]
    reg, hei, dim, rot, vel = R.split_heads(gold['head_maps'].astype(np.float32))
    return R.heat_of(gold['logits']), reg, hei, dim, rot, (vel if with_vel else None)


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(R.DECODE_CASES))
def test_decode_equals_the_reference_and_the_restatement(gold, case):
    import sst_amd
    norm_bbox = R.CASES[case][2]
    cfg = R.coder_cfg(case, float(gold['decode_score_threshold']))
    heat, reg, hei, dim, rot, vel = _decode_inputs(gold, case)
    r_boxes, r_scores, r_labels, r_keep = R.decode(heat, reg, hei, dim, rot, vel, cfg, norm_bbox)
    coder = sst_amd.CenterPointBBoxCoder(**cfg)
    g_rot = _t(rot)
    g_dim = _t(dim)
    args = (_t(heat), g_rot[:, 0:1], g_rot[:, 1:2], _t(hei), g_dim, None if vel is None else _t(vel))
    boxes, scores, clses, keep = (x.cpu().numpy() for x in coder.decode_batch(*args, reg=_t(reg), norm_bbox=norm_bbox))
    assert np.array_equal(scores, r_scores) and np.array_equal(clses, r_labels) and np.array_equal(keep, r_keep)
    plain = [0, 1, 2] + ([7, 8] if vel is not None else []) + ([] if norm_bbox else [3, 4, 5])
    assert np.array_equal(boxes[..., plain], r_boxes[..., plain])
    d = R.ulp_distance(boxes, r_boxes).max()
    print(f'{case}: exp / atan2 columns max ulp distance to the restatement {d}')
    assert d <= ULP_MATH
    # the reference's signature: dim as get_bboxes hands it over (exp applied where norm_bbox), a list of dicts per sample
    res = coder.decode(args[0], args[1], args[2], args[3], torch.exp(g_dim) if norm_bbox else g_dim, args[5], reg=_t(reg))
    for i, r in enumerate(res):
        order = np.argsort(-gold[f'decode_{case}_s{i}_scores'], kind='stable')
        mine = np.argsort(-r['scores'].cpu().numpy(), kind='stable')
        assert np.array_equal(r['scores'].cpu().numpy()[mine], gold[f'decode_{case}_s{i}_scores'][order])
        assert np.array_equal(r['labels'].cpu().numpy()[mine], gold[f'decode_{case}_s{i}_labels'][order])
        g_boxes, m_boxes = gold[f'decode_{case}_s{i}_bboxes'][order], r['bboxes'].cpu().numpy()[mine]
        assert m_boxes.shape == g_boxes.shape
        assert np.array_equal(m_boxes[:, plain], g_boxes[:, plain])
        assert R.ulp_distance(m_boxes, g_boxes).max() <= ULP_MATH


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['shipped', 'two_tasks'])
def test_get_bboxes_is_decode_then_the_rotated_nms(gold, case):
    import sst_amd
    from sst_amd import box_ops
    cfg, tasks, norm_bbox, _ = R.CASES[case]
    test_cfg = dict(nms_type='rotate', nms_thr=0.2, pre_max_size=40, post_max_size=12, score_threshold=0.9,
                    post_center_limit_range=[-4.8, -4.3, -2.53, 4.8, 4.3, 1.03])
    head = sst_amd.CenterHead(tasks=tasks, train_cfg=cfg, test_cfg=test_cfg, norm_bbox=norm_bbox,
                              bbox_coder=dict(type='CenterPointBBoxCoder', **R.coder_cfg('shipped', 0.1)))
    maps = {k: _t(v) for k, v in zip(HEADS, R.split_heads(gold['head_maps'].astype(np.float32)))}
    maps['dim'] = maps['dim'] * 0.25 + 0.5          # boxes of 1 to 3 m: they overlap
    logits, preds, at = _t(gold['logits']), [], 0
    for task in tasks:
        c = len(task['class_names'])
        preds.append([dict(maps, heatmap=logits[:, at:at + c].contiguous())])
        at += c
    got = head.get_bboxes(preds, [dict()] * 3)
    assert len(got) == 3
    total = 0
    for i in range(3):
        parts, flag = [], 0
        for task, pred in zip(tasks, preds):
            p = pred[0]
            boxes, scores, clses, keep = head.bbox_coder.decode_batch(p['heatmap'].sigmoid(), p['rot'][:, 0:1], p['rot'][:, 1:2],
                                                                      p['height'], p['dim'], p['vel'], reg=p['reg'],
                                                                      norm_bbox=norm_bbox)
            sel = keep[i] & (scores[i] >= test_cfg['score_threshold'])
            b, s, l = boxes[i][sel], scores[i][sel], clses[i][sel].long()
            kept = box_ops.nms_gpu(box_ops.xywhr2xyxyr(b[:, [0, 1, 3, 4, 6]]), s, test_cfg['nms_thr'],
                                   pre_maxsize=test_cfg['pre_max_size'], post_max_size=test_cfg['post_max_size'])
            assert 0 < kept.numel() < min(b.size(0), test_cfg['pre_max_size']), 'the NMS must suppress something'
            b, s, l = b[kept], s[kept], l[kept]
            rng = b.new_tensor(test_cfg['post_center_limit_range'])
            inside = (b[:, :3] >= rng[:3]).all(1) & (b[:, :3] <= rng[3:]).all(1)
            parts.append((b[inside], s[inside], (l[inside] + flag).int()))
            flag += len(task['class_names'])
        want_boxes = torch.cat([p[0] for p in parts])
        want_boxes[:, 2] = want_boxes[:, 2] - want_boxes[:, 5] * 0.5
        assert torch.equal(got[i][0], want_boxes)
        assert torch.equal(got[i][1], torch.cat([p[1] for p in parts]))
        assert torch.equal(got[i][2], torch.cat([p[2] for p in parts])) and got[i][2].dtype == torch.int32
        total += want_boxes.size(0)
        if len(tasks) == 2:
            assert (got[i][2] == 2).any() and (got[i][2] < 2).any()
    assert total > 6
