"""VoteSegHead's training side on the GPU (csrc/seg_loss.hip): the targets kernel against this library's own points-in-boxes,
the float32 restatement and the reference's golden; the loss kernels against float64 autograd of the restatement; the
segmentor's forward_train end to end.

Tolerances of the losses (float64 of the restatement on the same float32 inputs): relative error of each loss scalar and
max |err| / max |grad| of each gradient tensor <= max(4 * noise, 1e-6), noise = the reference's own float32-vs-float64 gap
stored in the golden (2e-8 .. 1e-7 for the losses, 2e-7 for the logit gradient, 1e-9 for the vote gradient): factor 4 for a
different but equally valid operation order and other exp / log routines, floor 1e-6 (about 16 float32 ulp) for a dozen rounded
operations and three transcendental calls per element.  Every case prints its errors before it asserts (pytest -s)."""
import ast
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

import seg_loss_ref as R

DEV = 'cuda:0'
WIDTHS = {'none': None, 'p02': 0.2, 'm03': -0.3}


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


# ---- targets -------------------------------------------------------------------------------------------------------

def _inside_points(rng, box, k, frac=0.35):
    """k points well inside a box: within frac of its length and width of the centre line, between 20 % and 80 % of its height"""
    return R.local_to_world(box, rng.uniform(-frac, frac, k) * box[4], rng.uniform(-frac, frac, k) * box[3],
                            rng.uniform(0.2, 0.8, k))


def _target_scene():
    """three samples; sample 0 crosses the box tile of the kernel and carries the orderings the issue names"""
    import sst_amd
    tile = sst_amd.seg_loss.seg_targets_box_tile()
    rng = np.random.default_rng(11)
    g0 = tile + 1
    b0 = np.zeros((g0, 7), np.float32)
    # filler boxes on a far grid that holds no point
    idx = np.arange(g0)
    b0[:, 0], b0[:, 1], b0[:, 2] = 200 + 6 * (idx % 20), 200 + 6 * (idx // 20), -1.0
    b0[:, 3:6], b0[:, 6] = np.float32([1.8, 4.2, 1.6]), rng.uniform(-3, 3, g0)
    b0[0] = [5, 5, -1, 2.0, 4.5, 1.7, 0.3]
    b0[1] = [5.5, 5.4, -1, 2.0, 4.5, 1.7, 0.5]          # overlaps box 0
    b0[2] = [-8, 3, -1.2, 1.9, 4.0, 1.6, -1.1]
    b0[3] = [-8.3, 3.5, -1.2, 1.9, 4.0, 1.6, -0.9]      # overlaps box 2
    b0[4] = [12, -9, -1, 2.1, 4.4, 1.5, 2.0]            # labelled -1, in front of ...
    b0[5] = b0[4]                                        # ... a valid box over the same points
    b0[6] = [-3, -12, -1, 0.5, 3.0, 1.6, 0.7]           # 0.5 m wide: keeps its extents at extra_width -0.3
    b0[g0 - 1] = [20, 20, -1, 2.0, 4.0, 1.6, -0.4]      # the LAST box, behind the tile boundary, alone over its points
    l0 = rng.integers(0, 3, g0).astype(np.int64)
    l0[4] = -1
    l0[5], l0[g0 - 1] = 2, 1
    n0 = 2 * 256 + 1
    parts = [_inside_points(rng, b0[k], 40) for k in (0, 1, 2, 3, 4, 6, g0 - 1)]
    parts += [np.float32([5.25, 5.2, -0.2]) + rng.normal(0, 0.15, (30, 3)).astype(np.float32),     # inside boxes 0 AND 1
              np.float32([-8.15, 3.25, -0.4]) + rng.normal(0, 0.15, (30, 3)).astype(np.float32)]  # inside boxes 2 AND 3
    placed = np.concatenate(parts)
    free = rng.uniform(-25, 25, (n0 - len(placed), 3)).astype(np.float32) * np.float32([1, 1, 0.1])
    p0 = np.concatenate([placed, free])[rng.permutation(n0)]
    b2 = np.float32([[2, 2, -1, 2, 4, 1.6, 0.2], [-4, 6, -1, 2, 4, 1.6, 1.2], [7, -7, -1, 2, 4, 1.6, -2.0]])
    l2 = np.int64([-1, -1, -1])
    p2 = np.concatenate([_inside_points(rng, b2[k], 16) for k in range(3)] + [rng.uniform(-9, 9, (16, 3)).astype(np.float32)])
    p1 = np.float32([[5.1, 5.1, -0.3]])                  # inside box 0 of sample 0: its own sample has no boxes
    boxes, labels = [b0, np.zeros((0, 7), np.float32), b2], [l0, np.zeros(0, np.int64), l2]
    points = []
    for p in (p0, p1, p2):
        everything = np.concatenate([b0, b2])
        bad = R.near_a_face(everything, p)
        while bad.any():       # nudge the few points that lie within 1 mm of a face plane
            p[bad] += rng.normal(0, 0.01, (int(bad.sum()), 3)).astype(np.float32)
            bad = R.near_a_face(everything, p)
        points.append(np.concatenate([p, rng.random((len(p), 2)).astype(np.float32)], 1))   # [N, 5] rows
    return points, boxes, labels


@pytest.fixture(scope='module')
def target_scene():
    return _target_scene()


@pytest.mark.gpu
@pytest.mark.parametrize('tag', list(WIDTHS))
def test_targets_of_a_batch(target_scene, tag):
    import sst_amd
    points, boxes, labels = target_scene
    width = WIDTHS[tag]
    lab, tgt, mask, inbox = sst_amd.seg_point_targets([_t(p) for p in points], [_t(b) for b in boxes],
                                                      [_t(l) for l in labels], 3, extra_width=width)
    n = sum(len(p) for p in points)
    assert lab.shape == (n,) and tgt.shape == (n, 3) and mask.shape == (n,) and inbox.shape == (n,)
    assert lab.dtype == torch.long and mask.dtype == torch.bool and inbox.dtype == torch.int32
    inbox_h = inbox.cpu().numpy()

    # the same membership as this library's points_in_boxes_gpu on each sample's filtered, enlarged boxes, mapped back
    p_off = np.cumsum([0] + [len(p) for p in points])
    b_off = np.cumsum([0] + [len(b) for b in boxes])
    for s in range(3):
        keep = np.nonzero(labels[s] >= 0)[0]
        want = np.full(len(points[s]), -1, np.int64)
        if len(keep):
            big = R.enlarge(boxes[s], width)[keep]
            first = sst_amd.points_in_boxes_gpu(_t(points[s][None, :, :3]), _t(big[None])).cpu().numpy()[0]
            want = np.where(first >= 0, keep[np.clip(first, 0, None)] + b_off[s], -1)
        assert np.array_equal(inbox_h[p_off[s]:p_off[s + 1]], want), f'sample {s}'

    # the orderings of sample 0: lower index wins an overlap, a box labelled -1 never wins, the last box is reached
    g0 = len(boxes[0])
    in0 = inbox_h[:p_off[1]]
    counts = np.bincount(in0[in0 >= 0], minlength=g0)
    assert counts[0] >= 60 and counts[2] >= 60, 'points in two boxes go to the lower index'
    assert counts[4] == 0 and counts[5] >= 35 and counts[g0 - 1] >= 35 and counts[6] >= 35
    assert (inbox_h[p_off[1]:] == -1).all(), 'samples without a valid box are background'

    rlab, rtgt, rmask, rinbox = R.point_targets(points, boxes, labels, 3, width)
    assert np.array_equal(inbox_h, rinbox)
    assert torch.equal(lab.cpu(), torch.from_numpy(rlab)) and torch.equal(mask.cpu(), torch.from_numpy(rmask))
    assert torch.equal(tgt.cpu(), torch.from_numpy(rtgt))
    if width == -0.3:
        assert (rinbox == 6).sum() >= 35


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['sig', 'ce'])
def test_targets_equal_the_reference_golden(case):
    import sst_amd
    gold = load_golden('seg_head_train.npz')
    key = 'labels3' if case == 'sig' else 'labels10'
    for tag, width in WIDTHS.items():
        lab, tgt, mask, _ = sst_amd.seg_point_targets(
            [_t(gold['points0']), _t(gold['points1'])], [_t(gold['boxes0']), _t(gold['boxes1'])],
            [_t(gold[f'{key}_0']), _t(gold[f'{key}_1'])], 3 if case == 'sig' else 10, extra_width=width)
        assert np.array_equal(lab.cpu().numpy(), gold[f'tgt_{case}_{tag}_labels'])
        assert np.array_equal(mask.cpu().numpy(), gold[f'tgt_{tag}_mask'])
        assert R.ulp_distance(tgt.cpu().numpy(), gold[f'tgt_{tag}_targets']).max() <= 1


@pytest.mark.gpu
def test_centroid_offset_targets(target_scene):
    import sst_amd
    from sst_amd.detectors import VoteSegHead
    points, boxes, labels = target_scene
    lab, tgt, mask, inbox = sst_amd.seg_point_targets([_t(p) for p in points], [_t(b) for b in boxes],
                                                      [_t(l) for l in labels], 3, centroid_offset=True)
    plain = sst_amd.seg_point_targets([_t(p) for p in points], [_t(b) for b in boxes], [_t(l) for l in labels], 3)
    assert torch.equal(lab, plain[0]) and torch.equal(mask, plain[2]) and torch.equal(inbox, plain[3])
    inbox_h, mask_h = inbox.cpu().numpy(), mask.cpu().numpy()
    centre = R.centroids64(points, boxes, inbox_h)
    xyz = np.concatenate([p[:, :3] for p in points]).astype(np.float64)
    want = np.where(mask_h[:, None], centre[np.clip(inbox_h, 0, None)] - xyz, 0.0)
    # the root is ill-conditioned at zero, the offset is not: compare the decoded offsets
    got = VoteSegHead.decode_vote_targets(tgt).cpu().numpy().astype(np.float64)
    assert np.abs(got - want).max() <= 1e-5
    assert np.abs(want[mask_h]).max() > 0.5 and not torch.equal(tgt, plain[1])


# ---- losses --------------------------------------------------------------------------------------------------------

LOSS_CASES = {
    'sig1': dict(mode=R.SIGMOID_FOCAL, c=1, gamma=2.0, alpha=0.25),
    'sig3': dict(mode=R.SIGMOID_FOCAL, c=3, gamma=3.0, alpha=0.8),
    'sig3_gamma1.5': dict(mode=R.SIGMOID_FOCAL, c=3, gamma=1.5, alpha=0.6),
    'ce2': dict(mode=R.SOFTMAX_CE, c=2, weights=False),
    'ce2w': dict(mode=R.SOFTMAX_CE, c=2, weights=True),
    'ce11': dict(mode=R.SOFTMAX_CE, c=11, weights=False),
    'ce11w': dict(mode=R.SOFTMAX_CE, c=11, weights=True),
    'ce27': dict(mode=R.SOFTMAX_CE, c=27, weights=False),
    'ce27w': dict(mode=R.SOFTMAX_CE, c=27, weights=True),
}


def _loss_kwargs(spec):
    c = spec['c']
    if spec['mode'] == R.SIGMOID_FOCAL:
        return dict(mode=spec['mode'], gamma=spec['gamma'], alpha=spec['alpha'], score_thresh=[0.3, 0.25, 0.25][:c])
    if c == 11:
        groups, thr = R.class_group(R.NUSC_CLASS_NAMES, R.NUSC_GROUP_NAMES), R.NUSC_SCORE_THRESH
        weight = R.NUSC_CLASS_WEIGHT
    else:
        n_groups = min(c - 1, 8)
        groups = [k % n_groups for k in range(c - 1)]
        if c > 3:
            groups[3] = -1                       # a class in no group
        thr = [0.1 + 0.05 * (g % 3) for g in range(n_groups)]
        weight = [0.5 + 0.25 * (k % 5) for k in range(c - 1)] + [0.1]
    return dict(mode=spec['mode'], class_weight=weight if spec['weights'] else None, score_thresh=thr, class_group=groups)


def _tolerances(mode):
    gold = load_golden('seg_head_train.npz')
    case = 'sig' if mode == R.SIGMOID_FOCAL else 'ce'
    return {k: max(4.0 * float(gold[f'noise_{case}_{k}'].max()), 1e-6)
            for k in ('loss_sem_seg', 'loss_vote', 'd_logits', 'd_vote_preds')}


def _loss_inputs(n, c, mode, scale, kw, seed, masked='some'):
    """float32 inputs with the required cases in them; every score at least 1e-4 from its threshold"""
    rng = np.random.default_rng(seed)
    hi = c + 1 if mode == R.SIGMOID_FOCAL else c               # sigmoid: label c is the background
    labels = rng.integers(0, hi, n)
    if mode == R.SOFTMAX_CE:
        labels[rng.random(n) < 0.5] = c - 1                    # mostly background, as in a frame
    labels[:min(n, hi)] = np.arange(hi)[:min(n, hi)]            # every label occurs when there is room
    if n == 1:
        # the single row starts (60, -60, ...): with label 0 the whole float64 gradient is of the order exp(-120), below
        # float32's range, and a relative error against it says nothing; label 1 puts the row's gradient at order 1
        labels[0] = 1
    n_fg = c if mode == R.SIGMOID_FOCAL else c - 1
    is_fg = labels < n_fg
    if masked == 'all':
        labels = rng.integers(0, c, n)
        mask = np.ones(n, bool)
    elif masked == 'none':
        mask = np.zeros(n, bool)
    else:
        mask = is_fg & (rng.random(n) < 0.8)
        if n > 2:
            mask[:hi][is_fg[:hi]] = True
    special = np.float32([60, -60, 0, 1e-3, -1e-3])

    def draw():
        x = rng.normal(0, 2.0, (n, c)).astype(np.float32)
        k = min(n, 40)
        x[:k] = special[(np.arange(k)[:, None] + np.arange(c)[None]) % 5] / np.float32(scale)
        return x

    logits = draw()
    for _ in range(50):
        z = torch.from_numpy(logits).double() * scale
        if mode == R.SIGMOID_FOCAL:
            gap = (torch.sigmoid(z) - torch.tensor(kw['score_thresh'], dtype=torch.float64)[None]).abs().min(1)[0]
        else:
            prob = torch.softmax(z, 1)[:, :-1]
            grp = torch.tensor(kw['class_group'])
            gs = torch.stack([prob[:, grp == g].sum(1) for g in range(len(kw['score_thresh']))], 1)
            gap = (gs - torch.tensor(kw['score_thresh'], dtype=torch.float64)[None]).abs().min(1)[0]
        bad = (gap < 1e-4).numpy()
        if not bad.any():
            break
        logits[bad] = rng.normal(0, 2.0, (int(bad.sum()), c)).astype(np.float32)
    assert not bad.any(), 'a score stayed within 1e-4 of its threshold'
    votes = rng.normal(0, 1.0, (n, 3 * c)).astype(np.float32)      # different values per class: a wrong gather shows
    targets = np.where(mask[:, None], rng.normal(0, 1.2, (n, 3)), 0).astype(np.float32)
    exact = np.nonzero(mask & (labels < c))[0][::3]                # some predictions equal their target: gradient 0
    for d in range(3):
        votes[exact, 3 * labels[exact] + d] = targets[exact, d]
    return logits, votes, labels.astype(np.int64), targets, mask


def _run(logits, votes, labels, targets, mask, scale, kw, w_sem=2.0, w_vote=3.0):
    import sst_amd
    lg = _t(logits).requires_grad_(True)
    vp = _t(votes).requires_grad_(True)
    out = sst_amd.seg_vote_loss(lg, vp, _t(labels), _t(targets), _t(mask), logit_scale=scale, **kw)
    (w_sem * out[0] + w_vote * out[1]).backward()
    return dict(loss_sem=out[0].detach(), loss_vote=out[1].detach(), recall=out[2], num_fg=out[3], counts=out[4],
                d_logits=lg.grad, d_vote_preds=vp.grad)


def _check(got, ref, tol, c, mode, what, report=None):
    counts = got['counts'].cpu().numpy()
    assert counts[0] == ref['num_valid'] and counts[1] == ref['status'], what
    assert np.array_equal(counts[2:2 + c], ref['tp'].numpy()) and np.array_equal(counts[2 + c:], ref['real'].numpy()), what
    assert int(got['num_fg'].item()) == ref['num_fg'], what
    assert torch.allclose(got['recall'].cpu(), ref['recall'], rtol=1e-6, atol=0), what
    errs = {}
    for key, tkey in (('loss_sem', 'loss_sem_seg'), ('loss_vote', 'loss_vote')):
        value = float(got[key].double().item())
        assert np.isfinite(value), what
        errs[tkey] = abs(value - ref[key]) / abs(ref[key]) if ref[key] != 0 else abs(value)
    for key in ('d_logits', 'd_vote_preds'):
        g = got[key].cpu().double()
        assert torch.isfinite(g).all(), what
        top = float(ref[key].abs().max())
        errs[key] = float((g - ref[key]).abs().max()) / top if top > 0 else float(g.abs().max())
    print(f'{what}: ' + ', '.join(f'{k} {v:.2e} (tol {tol[k]:.1e})' for k, v in errs.items()))
    if report is not None:
        for k, v in errs.items():
            report[k] = max(report.get(k, 0.0), v)
    for k, v in errs.items():
        assert v <= tol[k], f'{what}: {k} error {v:.3e} > {tol[k]:.1e}'


@pytest.mark.gpu
@pytest.mark.parametrize('scale', [1.0, 0.5])
@pytest.mark.parametrize('name', list(LOSS_CASES))
def test_losses_and_gradients_against_float64(name, scale):
    import sst_amd
    spec = LOSS_CASES[name]
    kw, c, mode = _loss_kwargs(spec), spec['c'], spec['mode']
    tol = _tolerances(mode)
    t = sst_amd.seg_loss.seg_loss_tile_rows()
    for n in (1, t, 2 * t + 1):
        inputs = _loss_inputs(n, c, mode, scale, kw, seed=n + c)
        got = _run(*inputs, scale, kw)
        ref = R.losses_and_grads(*(torch.from_numpy(a) for a in inputs), w_sem=2.0, w_vote=3.0, logit_scale=scale, **kw)
        assert ref['status'] == 0
        _check(got, ref, tol, c, mode, f'{name} scale {scale} n {n}')
        if n > 1:
            picked = np.nonzero(inputs[4])[0][::3]      # pred == target exactly: the L1 gradient is 0 there
            gv = got['d_vote_preds'].cpu().numpy().reshape(n, c, 3)
            assert (gv[picked, inputs[2][picked]] == 0).all()
            assert (got['d_vote_preds'] != 0).sum().item() > 0
        again = _run(*inputs, scale, kw)                # the same call twice: bit for bit
        for key in ('loss_sem', 'loss_vote', 'recall', 'num_fg', 'counts', 'd_logits', 'd_vote_preds'):
            assert torch.equal(got[key], again[key]), key


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['sig3', 'ce11w'])
def test_no_masked_point_and_every_point_masked(name):
    spec = LOSS_CASES[name]
    kw, c, mode = _loss_kwargs(spec), spec['c'], spec['mode']
    tol = _tolerances(mode)
    n = 700
    inputs = _loss_inputs(n, c, mode, 1.0, kw, seed=5, masked='none')
    got = _run(*inputs, 1.0, kw)
    assert float(got['loss_vote']) == 0.0 and int(got['counts'][0]) == 0
    assert (got['d_vote_preds'] == 0).all() and torch.isfinite(got['d_logits']).all() and torch.isfinite(got['loss_sem'])
    ref = R.losses_and_grads(*(torch.from_numpy(a) for a in inputs), w_sem=2.0, w_vote=3.0, **kw)
    _check(got, ref, tol, c, mode, f'{name} no masked point')
    inputs = _loss_inputs(n, c, mode, 1.0, kw, seed=6, masked='all')
    got = _run(*inputs, 1.0, kw)
    assert int(got['counts'][0]) == n
    ref = R.losses_and_grads(*(torch.from_numpy(a) for a in inputs), w_sem=2.0, w_vote=3.0, **kw)
    _check(got, ref, tol, c, mode, f'{name} every point masked')
    assert ((got['d_vote_preds'] != 0).sum(1) <= 3).all()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['sig3', 'ce11'])
def test_status_bits_replace_the_asserts(name):
    import sst_amd
    spec = LOSS_CASES[name]
    kw, c, mode = _loss_kwargs(spec), spec['c'], spec['mode']
    tol = _tolerances(mode)
    n = 300
    logits, votes, labels, targets, mask = _loss_inputs(n, c, mode, 1.0, kw, seed=9)
    bg = c if mode == R.SIGMOID_FOCAL else c - 1
    for bad_label, bad_mask, bits in ((c + 3, False, 1), (-2, False, 1), (c + 3, True, 3), (None, True, 2)):
        lab, msk = labels.copy(), mask.copy()
        if bad_label is not None:
            lab[17] = bad_label
            msk[17] = bad_mask
        elif mode == R.SIGMOID_FOCAL:
            lab[17], msk[17] = bg, True               # a masked background point
        else:
            continue                                  # the softmax head's background IS a class: the reference accepts it
        got = _run(logits, votes, lab, targets, msk, 1.0, kw)
        ref = R.losses_and_grads(*(torch.from_numpy(a) for a in (logits, votes, lab, targets, msk)), w_sem=2.0, w_vote=3.0,
                                 **kw)
        assert int(got['counts'][1]) == bits == ref['status']
        _check(got, ref, tol, c, mode, f'{name} label {bad_label} masked {bad_mask}')
        assert (got['d_logits'][17] == 0).all() or bad_label is None
        assert (got['d_vote_preds'][17] == 0).all()
    from sst_amd.detectors import VoteSegHead
    head = VoteSegHead(in_channel=8, num_classes=3, dropout_ratio=0.0,
                       loss_decode=dict(type='FocalLoss', use_sigmoid=True), loss_vote=dict(type='L1Loss'))
    head.train_cfg = dict(score_thresh=(0.3, 0.25, 0.25), class_names=('Car', 'Ped', 'Cyc'))
    lab = torch.tensor([0, 1, 7, 3], device=DEV)
    head.losses(torch.zeros(4, 3, device=DEV), torch.zeros(4, 9, device=DEV), lab, torch.zeros(4, 3, device=DEV),
                torch.zeros(4, dtype=torch.bool, device=DEV))
    with pytest.raises(AssertionError):
        head.check_status()


@pytest.mark.gpu
def test_loss_inputs_fail_loudly():
    import sst_amd
    n, c = 8, 3
    good = dict(logits=torch.zeros(n, c, device=DEV), vote_preds=torch.zeros(n, 3 * c, device=DEV),
                labels=torch.zeros(n, dtype=torch.long, device=DEV), vote_targets=torch.zeros(n, 3, device=DEV),
                vote_mask=torch.zeros(n, dtype=torch.bool, device=DEV))
    sst_amd.seg_vote_loss(*good.values(), mode=0)
    for key, bad in (('logits', torch.zeros(c, n, device=DEV).t()), ('logits', good['logits'].double()),
                     ('vote_preds', torch.zeros(n, 3 * c + 1, device=DEV)), ('labels', good['labels'].int()),
                     ('vote_targets', good['vote_targets'].half())):
        args = dict(good)
        args[key] = bad
        with pytest.raises(RuntimeError):
            sst_amd.seg_vote_loss(*args.values(), mode=0)


@pytest.mark.gpu
def test_large_launch_grid_arithmetic():
    spec = LOSS_CASES['sig3']
    kw, tol = _loss_kwargs(spec), _tolerances(R.SIGMOID_FOCAL)
    n, c = 300001, 3
    rng = np.random.default_rng(3)
    logits = rng.normal(0, 2.0, (n, c)).astype(np.float32)
    gap = np.abs(1 / (1 + np.exp(-logits.astype(np.float64))) - np.float64(kw['score_thresh'])[None]).min(1)
    logits[gap < 1e-4] = 3.0
    labels = rng.integers(0, c + 1, n).astype(np.int64)
    mask = (labels < c) & (rng.random(n) < 0.7)
    votes = rng.normal(0, 1.0, (n, 3 * c)).astype(np.float32)
    targets = np.where(mask[:, None], rng.normal(0, 1.2, (n, 3)), 0).astype(np.float32)
    inputs = (logits, votes, labels, targets, mask)
    got = _run(*inputs, 1.0, kw)
    ref = R.losses_and_grads(*(torch.from_numpy(a) for a in inputs), w_sem=2.0, w_vote=3.0, **kw)
    _check(got, ref, tol, c, R.SIGMOID_FOCAL, f'sig3 n {n}')
    assert (got['d_logits'][-1] != 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['sig', 'ce'])
def test_losses_on_the_reference_golden(case):
    """the reference's own float64 run (tests/golden/seg_head_train.npz) as the expected value"""
    gold = load_golden('seg_head_train.npz')
    mode = R.SIGMOID_FOCAL if case == 'sig' else R.SOFTMAX_CE
    if case == 'sig':
        kw, names = dict(mode=mode, gamma=3.0, alpha=0.8, score_thresh=(0.3, 0.25, 0.25)), ['Car', 'Ped', 'Cyc']
    else:
        kw = dict(mode=mode, class_weight=R.NUSC_CLASS_WEIGHT, score_thresh=R.NUSC_SCORE_THRESH,
                  class_group=R.class_group(R.NUSC_CLASS_NAMES, R.NUSC_GROUP_NAMES))
        names = R.NUSC_CLASS_NAMES
    tol = _tolerances(mode)
    got = _run(gold[f'{case}_logits'].astype(np.float32), gold[f'{case}_vote_preds'].astype(np.float32),
               gold[f'tgt_{case}_none_labels'], gold['tgt_none_targets'], gold['tgt_none_mask'], 1.0, kw, 1.0, 1.0)
    for key, gkey in (('loss_sem', 'loss_sem_seg'), ('loss_vote', 'loss_vote')):
        want = float(gold[f'{case}_f64_{gkey}'][0])
        assert abs(float(got[key].double()) - want) <= tol[gkey] * abs(want)
    for key in ('d_logits', 'd_vote_preds'):
        want = gold[f'{case}_f64_{key}']
        assert np.abs(got[key].cpu().numpy().astype(np.float64) - want).max() <= tol[key] * np.abs(want).max()
    recall = got['recall'].cpu().numpy()
    for k, name in enumerate(names):
        assert abs(recall[k] - float(gold[f'{case}_f32_recall_{name}'][0])) <= 1e-6 * recall[k]
    if case == 'ce':
        assert float(got['num_fg']) == float(gold['ce_f64_num_fg'][0])


# ---- the segmentor, end to end -------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_vote_segmentor_forward_train_end_to_end():
    import bench_workloads as BW
    import sst_amd
    path = os.path.join(GOLDEN, 'configs', 'fsd', 'fsd_waymoD1_1x.model.py')
    cfg = ast.literal_eval(open(path).read())['segmentor']
    torch.manual_seed(0)
    seg = sst_amd.build_detector(cfg).to(DEV).train()
    clouds = [BW.chain_cloud(3000, 5, half_extent=12.0).to(DEV), BW.chain_cloud(2900, 6, half_extent=12.0).to(DEV)]
    boxes, labels = [], []
    for s, cloud in enumerate(clouds):                 # three boxes per sample around object points
        centre = cloud[[len(cloud) - 1, len(cloud) - 300, len(cloud) - 700], :3].cpu()
        b = torch.zeros(3, 7)
        b[:, :2], b[:, 2] = centre[:, :2], centre[:, 2] - 0.8
        b[:, 3:6], b[:, 6] = torch.tensor([1.6, 3.0, 1.6]), torch.tensor([0.3, -1.0, 2.0]) + s
        boxes.append(b.to(DEV))
        labels.append(torch.tensor([0, 1, 2], device=DEV))
    losses = seg.forward_train([c.clone() for c in clouds], None, boxes, labels)
    assert set(losses) == {'loss_sem_seg', 'loss_vote', 'recall_Car', 'recall_Ped', 'recall_Cyc'}
    seg.segmentation_head.check_status()

    out = seg([c.clone() for c in clouds])             # train mode: batch statistics, the same features
    lab, tgt, mask = seg.segmentation_head.get_targets(seg.preprocess([c.clone() for c in clouds]), boxes, labels)
    assert int(mask.sum()) > 50
    ref = R.losses_and_grads(out['seg_logits'], out['seg_vote_preds'], lab, tgt, mask, R.SIGMOID_FOCAL, gamma=3.0,
                             alpha=0.8, score_thresh=(0.3, 0.25, 0.25))
    tol = _tolerances(R.SIGMOID_FOCAL)
    assert abs(float(losses['loss_sem_seg']) - ref['loss_sem']) <= tol['loss_sem_seg'] * abs(ref['loss_sem'])
    assert abs(float(losses['loss_vote']) - ref['loss_vote']) <= tol['loss_vote'] * abs(ref['loss_vote'])
    for k, name in enumerate(('Car', 'Ped', 'Cyc')):
        assert torch.allclose(losses[f'recall_{name}'].cpu(), ref['recall'][k], rtol=1e-6)

    (losses['loss_sem_seg'] + losses['loss_vote']).backward()
    for name, p in seg.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert seg.segmentation_head.conv_seg.weight.grad.abs().max() > 0
    assert seg.segmentation_head.voting.weight.grad.abs().max() > 0

    sub = seg.forward_train([c.clone() for c in clouds], None, boxes, labels, as_subsegmentor=True)
    assert set(sub) == set(out) | {'losses'}
    assert set(sub['losses']) == set(losses)
    assert torch.equal(sub['seg_points'], out['seg_points']) and sub['seg_logits'].shape == out['seg_logits'].shape
