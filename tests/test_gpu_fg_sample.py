"""The foreground sampling kernels (csrc/fg_sample.hip) on the GPU against the torch restatement of the reference's data flow
(tests/fsd_sample_ref.py, pinned to the reference by tests/test_fsd_sample_host.py) and against the golden cases.

Rules: masks, slots, sources, counts, rule flags, row orders, batch indices and every copied row are EQUAL (bit for bit for
floats); centres are one fp32 add, bit for bit; gradients on small-integer data are bit for bit against torch autograd of the
restatement, on real data within max(4 x the restatement's own fp32-vs-fp64 gap, 1e-6); a call repeated gives the same bits.
Every logit of a test keeps its float64 sigmoid 1e-6 away from the float32 threshold of its class (asserted)."""
import numpy as np
import pytest
import torch

import fsd_sample_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _fs():
    from sst_amd import fg_sample
    return fg_sample


def _bits(a, b, what):
    assert a.shape == b.shape, f'{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}'
    assert a.dtype == b.dtype, f'{what}: {a.dtype} vs {b.dtype}'
    if a.is_floating_point():
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), f'{what}: not bit for bit'
    else:
        assert torch.equal(a, b), f'{what}: not equal'


def _strided(t, left=1, right=2):
    """the same values as a column slice of a wider tensor: the row stride differs from the width"""
    wide = torch.cat([torch.full_like(t[:, :1], 7.).expand(-1, left), t, torch.full_like(t[:, :1], -7.).expand(-1, right)], 1)
    return wide[:, left:left + t.size(1)]


def _check_sample(data, thr, batch_size, extra=None, what=''):
    """fg_sample against the restatement; -> (kernel result, restatement result)"""
    FS = _fs()
    assert bool(R.margin_ok(data['seg_logits'], thr).all()), f'{what}: a logit is ambiguous against its threshold'
    got = FS.fg_sample(_strided(data['seg_logits']), data['vote_offsets'], data['seg_points'], data['batch_idx'], thr, batch_size,
                       extra_mask=extra, validate=True)
    want = R.sample(data, thr, extra)
    c, n = len(thr), data['seg_points'].size(0)
    assert got['rule'] == want['rule'], f'{what}: rule flags {got["rule"]} vs {want["rule"]}'
    assert got['totals'] == [int(m.sum()) for m in want['fg_mask_list']], f'{what}: totals'
    for k in range(c):
        mask = want['fg_mask_list'][k]
        _bits(got['fg_mask_list'][k], mask, f'{what}: mask of class {k}')
        _bits(got['seg_points'][k], want['seg_points'][k], f'{what}: seg_points of class {k}')
        _bits(got['batch_idx'][k], want['batch_idx'][k], f'{what}: batch_idx of class {k}')
        _bits(got['center_preds'][k], want['center_preds'][k], f'{what}: center_preds of class {k}')
        rows = torch.nonzero(mask)[:, 0]
        _bits(got['src'][k], rows.int(), f'{what}: src of class {k}')
        slot = torch.full((n,), -1, dtype=torch.int32, device=mask.device)
        slot[rows] = torch.arange(rows.numel(), dtype=torch.int32, device=mask.device)
        _bits(got['slot'][k], slot, f'{what}: slot of class {k}')
    return got, want


def _valid_masks(sampled, seed, keep=0.7):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(m.size(0), generator=g) < keep).to(m.device) for m in sampled['seg_points']]


def _check_gather(data, got, want, valid, what=''):
    FS = _fs()
    out = FS.fg_gather_cat(got, valid, _strided(data['seg_logits']), data['seg_vote_preds'], _strided(data['seg_feats'], 3, 1),
                           data['seg_points'])
    ref_upd = R.update_by_mask(want, valid)
    ref = R.combine(ref_upd)
    _bits(out['pts_feats'], ref['pts_feats'], f'{what}: pts_feats')
    _bits(out['seg_points'], ref['points'], f'{what}: combined points')
    _bits(out['center_preds'], ref['center_preds'], f'{what}: combined center_preds')
    for k, m in enumerate(ref_upd['fg_mask_list']):
        _bits(out['fg_mask_list'][k], m, f'{what}: final mask of class {k}')
    return out, ref_upd


def _check_roi(data, final_masks, slot2, seed, batch_size, what=''):
    FS = _fs()
    g = torch.Generator().manual_seed(seed)
    m = int(sum(int(x.sum()) for x in final_masks))
    cluster = torch.randn(m, 5, generator=g).to(DEV)
    pts, feats, bidx, _ = FS.roi_input(data['seg_points'], cluster, _strided(data['seg_feats']), final_masks, data['batch_idx'],
                                       batch_size, slot2=slot2)
    r_pts, r_feats, r_bidx = R.roi_multi(data['seg_points'], cluster, data['seg_feats'], final_masks, data['batch_idx'])
    _bits(bidx, r_bidx, f'{what}: roi batch inds')
    _bits(pts, r_pts, f'{what}: roi points')
    _bits(feats, r_feats, f'{what}: roi cat_feats')
    n_bg = int((torch.stack(list(final_masks)).sum(0) == 0).sum())
    pts2, feats2, bidx2, _ = FS.roi_input(data['seg_points'], cluster, data['seg_feats'], final_masks, data['batch_idx'], batch_size,
                                          num_rows=n_bg + m)                      # known counts, slots restated from the masks
    _bits(feats2, r_feats, f'{what}: roi cat_feats with known counts')
    _bits(pts2, r_pts, f'{what}: roi points with known counts')


SAMPLES = [(1, ()), (2, ()), (4, (1, 3)), (2, (1,)), (4, ())]        # (B, samples without a point: in the middle, at the end)
WIDTHS = [1, 3, 64, 67, 131]


@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 769, 1000])
def test_edge_sweep(n):
    """wave and workgroup tails, several blocks, C at both ends of the mask word, samples without points, odd widths, inputs
    whose row stride is not their width: sampling, the composed gather and the RoI input against the restatement"""
    for c in (1, 3, 32):
        for j, ((b, empty), f) in enumerate(zip(SAMPLES, WIDTHS)):
            what = f'n={n} C={c} B={b} empty={empty} F={f}'
            data, thr = R.make_case(n, c, b, f, seed=1000 * c + 10 * j + n, fg=0.3, empty_samples=empty, device=DEV)
            got, want = _check_sample(data, thr, b, what=what)
            valid = _valid_masks(want, seed=n + j)
            out, ref_upd = _check_gather(data, got, want, valid, what)
            if c < 32:
                _check_roi(data, ref_upd['fg_mask_list'], out['slot2'], n + c, b, what)


def test_empty_input_launches_nothing():
    FS = _fs()
    data, thr = R.make_case(0, 3, 2, 67, seed=1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = FS.fg_sample(data['seg_logits'], data['vote_offsets'], data['seg_points'], data['batch_idx'], thr, 2)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert got['totals'] == [0, 0, 0] and got['rule'] == [False] * 3
    assert all(t.shape == (0, 4) for t in got['seg_points']) and all(t.shape == (0, 3) for t in got['center_preds'])
    out = FS.fg_gather_cat(got, [torch.zeros(0, dtype=torch.long, device=DEV)] * 3, data['seg_logits'], data['seg_vote_preds'],
                           data['seg_feats'], data['seg_points'])
    assert out['pts_feats'].shape == (0, 3 + 9 + 67)


def test_rule_special_cases():
    """the rule fires because one (class, sample) pair is empty, with a first point that was already selected in another sample;
    a class that selects nothing before the rule; a class that selects everything; a threshold buffer; unsorted input is
    refused under validate"""
    FS = _fs()
    data, thr = R.make_case(700, 3, 3, 8, seed=5, fg=0.4, device=DEV)
    lg = data['seg_logits']
    s1 = data['batch_idx'] == 1
    first = [int(torch.nonzero(data['batch_idx'] == s)[0, 0]) for s in range(3)]
    lg[s1, 0] = -3.0                     # class 0 selects nothing in sample 1 ...
    lg[first[0], 0] = 3.0                # ... and the first point of sample 0 is selected already
    lg[first[2], 0] = -3.0
    lg[:, 1] = -5.0                      # class 1 selects nothing at all
    lg[:, 2] = 5.0                       # class 2 selects everything
    got, want = _check_sample(data, thr, 3, what='rule cases')
    assert got['rule'] == [True, True, False]
    assert got['totals'][1] == 3 and got['totals'][2] == 700
    thr_b = R.thresholds32([0.5, 0.3, 0.6], threshold_buffer=0.1)
    data2, _ = R.make_case(500, 3, 2, 8, seed=6, device=DEV)
    data2['seg_logits'] = R.redraw_until_clear(data2['seg_logits'].cpu(), thr_b).to(DEV)
    assert FS.round_thresholds([0.5, 0.3, 0.6], 0.1) == thr_b
    _check_sample(data2, thr_b, 2, what='threshold buffer')
    with pytest.raises(RuntimeError, match='non-decreasing'):
        FS.fg_sample(data2['seg_logits'], data2['vote_offsets'], data2['seg_points'], data2['batch_idx'].flip(0), thr_b, 2,
                     validate=True)
    with pytest.raises(RuntimeError, match='outside'):
        FS.fg_sample(data2['seg_logits'], data2['vote_offsets'], data2['seg_points'], data2['batch_idx'] + 1, thr_b, 2)
    with pytest.raises(NotImplementedError, match='classes'):
        FS.fg_sample(None, None, data2['seg_points'], data2['batch_idx'], [0.5] * 33, 2,
                     extra_mask=torch.zeros((33, 500), dtype=torch.bool, device=DEV))


def test_topk_and_gt_points():
    """the disable_pretrain state (top-k per class replaces the threshold; distinct scores) and add_gt_fg_points"""
    FS = _fs()
    from sst_amd import box_ops
    data, thr = R.make_case(900, 3, 2, 8, seed=9, device=DEV)
    assert all(data['seg_logits'][:, k].unique().numel() == 900 for k in range(3)), 'top-k inputs need pairwise distinct scores'
    topks = [100, 50, 1000]
    extra = FS.topk_extra_mask(data['seg_logits'], topks)
    _bits(extra, R.topk_extra_mask(data['seg_logits'], topks), 'top-k mask')
    inf = [float('inf')] * 3
    got, _ = _check_sample(data, inf, 2, extra, 'top-k')
    assert got['totals'][2] == 900 and got['totals'][1] in (50, 51, 52)
    # ground-truth boxes around some points, per sample as the reference does it (:776-794)
    g = torch.Generator().manual_seed(3)
    boxes, labels = [], []
    for s in range(2):
        rows = torch.nonzero(data['batch_idx'] == s)[:, 0]
        pick = rows[torch.randperm(rows.numel(), generator=g)[:6].to(DEV)]
        ctr = data['seg_points'][pick, :3]
        box = torch.cat([ctr[:, :2], ctr[:, 2:3] - 2., torch.full((6, 3), 6., device=DEV), torch.rand(6, 1, generator=g).to(DEV)], 1)
        boxes.append(box)
        labels.append(torch.tensor([0, 1, 2, 0, -1, 1], device=DEV))
    extra = FS.gt_extra_mask(data['seg_points'], data['batch_idx'], boxes, labels, 3)
    want = torch.zeros_like(extra)
    for s in range(2):
        mine = data['batch_idx'] == s
        for k in range(3):
            sel = boxes[s][labels[s] == k]
            want[k, mine] = box_ops.points_in_boxes_gpu(data['seg_points'][mine, :3][None].contiguous(), sel[None].contiguous())[0] > -1
    _bits(extra, want, 'ground-truth point mask')
    assert int(extra.sum()) >= 10
    _check_sample(data, thr, 2, extra, 'add_gt_fg_points')


def _flow_ref(data, thr, valid, w_pts, cluster, w_roi, dtype):
    """the restatement end to end in ``dtype`` -> gradients of seg_feats (through both uses) and of the cluster features"""
    d = {k: (v.to(dtype) if v.is_floating_point() and k != 'seg_logits' else v) for k, v in data.items()}
    feats = d['seg_feats'].clone().requires_grad_(True)
    d['seg_feats'] = feats
    clu = cluster.to(dtype).clone().requires_grad_(True)
    smp = R.sample(d, thr)
    upd = R.update_by_mask(smp, valid)
    comb = R.combine(upd)
    loss = (comb['pts_feats'].to(dtype) * w_pts.to(dtype)).sum()
    _, cat_feats, _ = R.roi_multi(d['seg_points'], clu, feats, upd['fg_mask_list'], d['batch_idx'])
    loss = loss + (cat_feats * w_roi.to(dtype)).sum()
    loss.backward()
    return feats.grad, clu.grad


def _flow_kernels(data, thr, valid, w_pts, cluster, w_roi, batch_size, **detach):
    FS = _fs()
    feats = data['seg_feats'].clone().requires_grad_(True)
    clu = cluster.clone().requires_grad_(True)
    smp = FS.fg_sample(data['seg_logits'], data['vote_offsets'], data['seg_points'], data['batch_idx'], thr, batch_size)
    out = FS.fg_gather_cat(smp, valid, data['seg_logits'], data['seg_vote_preds'], feats, data['seg_points'])
    loss = (out['pts_feats'] * w_pts).sum()
    _, cat_feats, _, _ = FS.roi_input(data['seg_points'], clu, feats, out['fg_mask_list'], data['batch_idx'], batch_size,
                                      slot2=out['slot2'], **detach)
    loss = loss + (cat_feats * w_roi).sum()
    loss.backward()
    return feats.grad, clu.grad, out


@pytest.mark.parametrize('integer', [True, False])
def test_gradients(integer):
    c, f, fc, b = 3, 67, 5, 2
    data, thr = R.make_case(777, c, b, f, seed=21, fg=0.45, int_feats=integer, device=DEV)
    masks, _ = R.fg_masks(data['seg_logits'], data['batch_idx'], thr)
    per_point = masks.sum(0)
    assert all(bool((per_point == k).any()) for k in (0, 1, 2, c)), 'points selected by 0, 1, 2 and all C classes are needed'
    want_s = R.sample(data, thr)
    valid = _valid_masks(want_s, seed=4, keep=0.8)
    m = int(sum(int(v.sum()) for v in valid))
    g = torch.Generator().manual_seed(8)
    draw = (lambda *s: torch.randint(-4, 5, s, generator=g).float()) if integer else (lambda *s: torch.randn(*s, generator=g))
    n_bg = int((torch.stack(R.update_by_mask(want_s, valid)['fg_mask_list']).sum(0) == 0).sum())
    w_pts, cluster, w_roi = draw(m, c + 3 * c + f).to(DEV), draw(m, fc).to(DEV), draw(n_bg + m, fc + f).to(DEV)
    g_feats, g_clu, _ = _flow_kernels(data, thr, valid, w_pts, cluster, w_roi, b)
    again = _flow_kernels(data, thr, valid, w_pts, cluster, w_roi, b)
    _bits(g_feats, again[0], 'seg_feats gradient of a repeated call')
    _bits(g_clu, again[1], 'cluster feature gradient of a repeated call')
    r32 = _flow_ref(data, thr, valid, w_pts, cluster, w_roi, torch.float32)
    if integer:
        _bits(g_feats, r32[0], 'seg_feats gradient on integer data')
        _bits(g_clu, r32[1], 'cluster feature gradient on integer data')
        return
    r64 = _flow_ref(data, thr, valid, w_pts, cluster, w_roi, torch.float64)
    for name, got, a32, a64 in (('seg_feats', g_feats, r32[0], r64[0]), ('cluster_pts_feats', g_clu, r32[1], r64[1])):
        gap = float((a32.double() - a64).abs().max())
        err = float((got.double() - a64).abs().max())
        bound = max(4 * gap, 1e-6)
        print(f'{name} gradient: error {err:.3e} against float64, the restatement\'s own gap {gap:.3e}, bound {bound:.3e}')
        assert err <= bound
    # the detach keys: no gradient reaches the detached input, the other one is unchanged
    gf, gc, _ = _flow_kernels(data, thr, valid, w_pts, cluster, w_roi, b, detach_cluster_feats=True)
    assert gc is None
    _bits(gf, g_feats, 'seg_feats gradient with detach_cluster_feats')
    gf, gc, _ = _flow_kernels(data, thr, valid, torch.zeros_like(w_pts), cluster, w_roi, b, detach_seg_feats=True)
    _bits(gc, g_clu, 'cluster gradient with detach_seg_feats')
    assert not bool(gf.any()), 'with detach_seg_feats the RoI input sends nothing to seg_feats'
    FS = _fs()
    feats = data['seg_feats'].clone().requires_grad_(True)
    smp = FS.fg_sample(data['seg_logits'], data['vote_offsets'], data['seg_points'], data['batch_idx'], thr, b)
    out = FS.fg_gather_cat(smp, valid, data['seg_logits'], data['seg_vote_preds'], feats, data['seg_points'], detach_feats=True)
    assert not out['pts_feats'].requires_grad


def test_single_class_roi_input():
    """C = 1 and prepare_roi_input: pad in place, no reordering; forward rows and both gradients on integer data"""
    FS = _fs()
    data, thr = R.make_case(515, 1, 3, 67, seed=31, fg=0.35, int_feats=True, device=DEV)
    got, want = _check_sample(data, thr, 3, what='C=1')
    valid = _valid_masks(want, seed=2)
    out, upd = _check_gather(data, got, want, valid, 'C=1')
    m = int(valid[0].sum())
    g = torch.Generator().manual_seed(1)
    cluster = torch.randint(-4, 5, (m, 6), generator=g).float().to(DEV)
    w = torch.randint(-4, 5, (515, 6 + 67), generator=g).float().to(DEV)
    grads = []
    for fn, masks in ((FS.roi_input_single, out['fg_mask_list']), (R.roi_single, upd['fg_mask_list'])):
        feats, clu = data['seg_feats'].clone().requires_grad_(True), cluster.clone().requires_grad_(True)
        pts, cat_feats, bidx = fn(data['seg_points'], clu, feats, masks, data['batch_idx'])
        (cat_feats * w).sum().backward()
        grads.append((pts, cat_feats.detach(), bidx, feats.grad, clu.grad))
    for name, a, b in zip(('points', 'cat_feats', 'batch_idx', 'd seg_feats', 'd cluster_pts_feats'), *grads):
        _bits(a, b, f'prepare_roi_input: {name}')


def test_no_host_synchronisation():
    """fg_sample_launch, fg_gather_cat forward and backward, roi_input forward and backward with known counts: nothing waits
    for the device"""
    FS = _fs()
    c, b, f = 3, 2, 67
    data, thr = R.make_case(1000, c, b, f, seed=41, device=DEV)
    want = R.sample(data, thr)
    valid = _valid_masks(want, seed=3)
    keeps = [torch.nonzero(v)[:, 0] for v in valid]
    upd = R.update_by_mask(want, valid)
    m = sum(k.numel() for k in keeps)
    n_bg = int((torch.stack(upd['fg_mask_list']).sum(0) == 0).sum())
    cluster = torch.randn(m, 5, device=DEV, requires_grad=True)
    feats = data['seg_feats'].clone().requires_grad_(True)
    smp = FS.fg_sample(data['seg_logits'], data['vote_offsets'], data['seg_points'], data['batch_idx'], thr, b)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        pend = FS.fg_sample_launch(data['seg_logits'], data['vote_offsets'], data['seg_points'], data['batch_idx'], thr, b)
        out = FS.fg_gather_cat(smp, keeps, data['seg_logits'], data['seg_vote_preds'], feats, data['seg_points'])
        pts, cat_feats, bidx, _ = FS.roi_input(data['seg_points'], cluster, feats, out['fg_mask_list'], data['batch_idx'], b,
                                               slot2=out['slot2'], num_rows=n_bg + m)
        (out['pts_feats'].sum() + cat_feats.sum()).backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert pend.finish()['totals'] == smp['totals']
    _bits(out['pts_feats'], R.combine(upd)['pts_feats'], 'pts_feats queued without a read')
    assert cat_feats.shape == (n_bg + m, 5 + f) and bool(torch.isfinite(feats.grad).all())


@pytest.fixture(scope='module')
def gold():
    return load_golden('fsd_sample.npz')


def _g(array):
    return torch.from_numpy(np.ascontiguousarray(array))      # the file stores its matrices column-major


def _gold_case(gold, name):
    keys = ('seg_points', 'seg_logits', 'seg_vote_preds', 'seg_feats', 'batch_idx', 'vote_offsets')
    data = {k: _g(gold[f'{name}_{k}']).to(DEV) for k in keys}
    thr = [float(x) for x in gold[f'{name}_thr32']]
    extra = _g(gold[f'{name}_extra']).to(DEV) if f'{name}_extra' in gold else None
    return data, thr, extra


def test_golden_cases(gold):
    """every case of tests/golden/fsd_sample.npz (the reference's own methods) through the kernels"""
    FS = _fs()
    names = [str(x) for x in gold['cases']]
    assert len(names) >= 8
    for name in names:
        data, thr, extra = _gold_case(gold, name)
        c, b = data['seg_logits'].size(1), int(gold[f'{name}_batch'])
        assert bool(R.margin_ok(data['seg_logits'], thr).all()), f'{name}: a logit is ambiguous against its threshold'
        got = FS.fg_sample(data['seg_logits'], data['vote_offsets'], data['seg_points'], data['batch_idx'], thr, b, extra_mask=extra)
        assert got['rule'] == [bool(x) for x in gold[f'{name}_rule']], f'{name}: rule flags'
        for k in range(c):
            for key in ('seg_points', 'batch_idx', 'center_preds'):
                _bits(got[key][k], _g(gold[f'{name}_s_{key}_{k}']).to(DEV), f'{name}: {key} of class {k}')
            _bits(got['fg_mask_list'][k], _g(gold[f'{name}_s_fg_mask_{k}']).to(DEV), f'{name}: mask of class {k}')
        valid = [_g(gold[f'{name}_valid_{k}']).to(DEV) for k in range(c)]
        out = FS.fg_gather_cat(got, valid, data['seg_logits'], data['seg_vote_preds'], data['seg_feats'], data['seg_points'])
        _bits(out['pts_feats'], _g(gold[f'{name}_pts_feats']).to(DEV), f'{name}: pts_feats')
        _bits(out['seg_points'], _g(gold[f'{name}_points']).to(DEV), f'{name}: combined points')
        _bits(out['center_preds'], _g(gold[f'{name}_center_preds']).to(DEV), f'{name}: combined center_preds')
        for k in range(c):
            _bits(out['fg_mask_list'][k], _g(gold[f'{name}_final_mask_{k}']).to(DEV), f'{name}: final mask {k}')
        cluster = _g(gold[f'{name}_cluster_pts_feats']).to(DEV)
        if c == 1:
            pts, cat_feats, bidx = FS.roi_input_single(data['seg_points'], cluster, data['seg_feats'], out['fg_mask_list'],
                                                       data['batch_idx'])
        else:
            pts, cat_feats, bidx, _ = FS.roi_input(data['seg_points'], cluster, data['seg_feats'], out['fg_mask_list'],
                                                   data['batch_idx'], b, slot2=out['slot2'])
        _bits(pts, _g(gold[f'{name}_roi_points']).to(DEV), f'{name}: roi points')
        _bits(cat_feats, _g(gold[f'{name}_roi_feats']).to(DEV), f'{name}: roi cat_feats')
        _bits(bidx, _g(gold[f'{name}_roi_batch']).to(DEV), f'{name}: roi batch inds')
