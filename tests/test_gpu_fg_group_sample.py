"""csrc/fg_group_sample.hip on the device against tests/golden/fsdv2_sample.npz (the reference's own methods) and the torch
restatement (tests/fsdv2_sample_ref.py): masks, rows, rule and narrow rows are equal; the voted centres bit for bit wherever at
most two logits of a group tie (the weights 1 and 0.5 make the products exact), three-way ties within
8 * 2^-24 * (|p| + |scale| * sum |o_k|) of the float64 evaluation (seven roundings, each at most 2^-24 of a quantity no larger than
that sum).  Every case's grouped scores are (K + 8) * 2^-23 clear of the thresholds, so the masks do not depend on whose exp ran."""
import numpy as np
import pytest
import torch

import fsdv2_sample_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CASES, case_of = R.CASES, R.case_of
PC_RANGE = [-51.2, -51.2, -5, 51.2, 51.2, 3]


@pytest.fixture(scope='module')
def gold():
    return load_golden('fsdv2_sample.npz')


def _bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, f'{what}: {a.dtype} {tuple(a.shape)} vs {b.dtype} {tuple(b.shape)}'
    if a.is_floating_point():
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), f'{what}: not bit for bit'
    else:
        assert torch.equal(a, b), what


def _run(data, groups, thr, extra, scale, batch, **kw):
    from sst_amd import fg_group_sample as GS
    d = {k: v.to(DEV) for k, v in data.items()}
    out = GS.group_sample(d['seg_logits'], d['vote_offsets'], d['seg_points'], d['batch_idx'], groups, thr, batch, scale,
                          None if extra is None else extra.to(DEV), **kw)
    return d, out


def _check(d, out, ref, groups, scale, what):
    """the kernel's result against a restatement's result (lists per group on any device)"""
    g_n, n = len(groups), d['seg_points'].size(0)
    masks = torch.stack(ref['fg_mask_list']).to(DEV)
    _bits(torch.stack(out['fg_mask_list']), masks, f'{what}: masks')
    assert out['rule'] == ref['rule'], what
    assert out['totals'] == [int(m.sum()) for m in masks] and out['class_offsets'][-1] == int(masks.sum())
    cen64, bound, ties = R.centers_f64(d, groups, list(masks), scale)
    for g in range(g_n):
        rows = torch.nonzero(masks[g])[:, 0]
        _bits(out['src'][g].long(), rows, f'{what}: src of group {g}')
        slot = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        slot[rows] = torch.arange(rows.numel(), dtype=torch.int32, device=DEV)
        _bits(out['slot'][g], slot, f'{what}: slot of group {g}')
        _bits(out['batch_idx'][g], ref['batch_idx'][g].to(DEV), f'{what}: batch_idx of group {g}')
        _bits(out['seg_points'][g], ref['seg_points'][g].to(DEV), f'{what}: seg_points of group {g}')
        got, want = out['center_preds'][g], ref['center_preds'][g].to(DEV)
        exact = ties[g] <= 2
        _bits(got[exact], want[exact], f'{what}: centres of group {g} (ties <= 2)')
        assert bool(((got.double() - cen64[g]).abs() <= bound[g]).all()), f'{what}: centres of group {g} against float64'
    _bits(out['src_cat'].long(), torch.cat([torch.nonzero(m)[:, 0] for m in masks]), f'{what}: src_cat')
    return masks


@pytest.mark.parametrize('name', CASES)
def test_kernel_equals_the_reference(gold, name):
    from sst_amd import fg_group_sample as GS
    data, groups, thr, extra, scale, batched = case_of(gold, name)
    batch = int(gold[f'{name}_batch'])
    d, out = _run(data, groups, thr, extra, scale, batch)
    ref = dict(fg_mask_list=[torch.from_numpy(gold[f'{name}_s_fg_mask_{g}']) for g in range(len(groups))],
               rule=[bool(x) for x in gold[f'{name}_rule']])
    for key in ('seg_points', 'batch_idx', 'center_preds'):
        ref[key] = [torch.from_numpy(np.ascontiguousarray(gold[f'{name}_s_{key}_{g}'])) for g in range(len(groups))]
    _check(d, out, ref, groups, scale, name)
    # the restatement on the device agrees too (its softmax is the device's)
    on_dev = R.group_sample(d, groups, thr, scale, None if extra is None else extra.to(DEV), batched)
    _check(d, out, on_dev, groups, scale, f'{name} (device restatement)')
    if name == 'tie3':
        assert int(torch.cat(R.centers_f64(d, groups, on_dev['fg_mask_list'], scale)[2]).max()) == 3
    if extra is not None:
        _bits(GS.group_topk_extra_mask(d['seg_logits'], groups, [int(x) for x in gold[f'{name}_topks']]), extra.to(DEV), 'top-k mask')
    # the projector's rows in one gather, and the clipped centres: bit for bit against the restatement on the device; against the
    # reference's CPU run the copied columns and the clipped centres are equal and the offset columns within one unit in the last
    # place (torch divides a device tensor by the scalar 10 as a product with the float32 reciprocal, a CPU tensor by a division)
    rows, clipped = GS.virtual_rows(out, d['seg_feats'], d['seg_logits'], d['seg_points'], PC_RANGE)
    f = d['seg_feats'].size(1)
    three = torch.cat(R.centers_f64(d, groups, on_dev['fg_mask_list'], scale)[2]) > 2
    dev_rows, dev_clipped = R.virtual_input(R.combine(dict(on_dev, center_preds=out['center_preds'])), PC_RANGE)
    _bits(rows, dev_rows, f'{name}: the projector input (device restatement)')
    _bits(clipped, dev_clipped, f'{name}: clipped centres (device restatement)')
    want_c, want_o = (torch.from_numpy(np.ascontiguousarray(gold[f'{name}_{k}'])).to(DEV) for k in ('clipped', 'virtual_offset'))
    _bits(clipped[~three], want_c[~three], f'{name}: clipped centres')
    got_o = rows[:, f:f + 3][~three]
    assert bool(((got_o - want_o[~three]).abs() <= 2.0 ** -23 * want_o[~three].abs()).all()), f'{name}: offset columns'
    if name == 'nusc':
        want = torch.from_numpy(np.ascontiguousarray(gold['nusc_virtual_input'])).to(DEV)
        copied = [c for c in range(want.size(1)) if not f <= c < f + 3]
        _bits(rows[:, copied], want[:, copied], 'nusc: the copied columns of the projector input')


def _small(n, b=2, seed=5, k=11):
    groups, thr = R.groups_by_names(R.NUSC_GROUPS, R.NUSC_CLASSES), R.thresholds32(R.NUSC_THRESH)
    return R.make_case(n, k, b, 8, seed, groups, thr, fg=0.4), groups, thr


def test_edge_sizes_strides_and_index_types():
    from sst_amd import fg_group_sample as GS
    # N = 0: nothing launched, empty lists
    data, groups, thr = _small(0)
    d, out = _run(data, groups, thr, None, 1, 1)
    assert out['totals'] == [0] * 6 and out['rule'] == [False] * 6 and all(t.numel() == 0 for t in out['src'])
    rows, clipped = GS.virtual_rows(out, d['seg_feats'], d['seg_logits'], d['seg_points'], PC_RANGE)
    assert tuple(rows.shape) == (0, 8 + 3 + 11 + 2) and tuple(clipped.shape) == (0, 3)
    # N = 1: the rule gives every empty group the point
    data, groups, thr = _small(1, b=1)
    d, out = _run(data, groups, thr, None, 1, 1)
    ref = R.group_sample(d, groups, thr)
    _check(d, out, ref, groups, 1, 'N = 1')
    assert out['totals'] == [1] * 6 and any(out['rule'])
    # strided logits / votes / points (a column block of a wider matrix), int32 and int64 batch_idx; more than one block
    data, groups, thr = _small(700, b=3, seed=6)
    ref = R.group_sample({k: v.to(DEV) for k, v in data.items()}, groups, thr, 0.3)
    wide = {k: torch.cat([torch.full((700, 3), 7.0), data[k], torch.full((700, 2), -7.0)], 1).to(DEV)[:, 3:-2]
            for k in ('seg_logits', 'vote_offsets', 'seg_points')}
    assert not wide['seg_logits'].is_contiguous()
    for dtype in (torch.int32, torch.int64):
        bidx = data['batch_idx'].to(DEV, dtype)
        out = GS.group_sample(wide['seg_logits'], wide['vote_offsets'], wide['seg_points'], bidx, groups, thr, 3, 0.3, validate=True)
        d = dict({k: v.to(DEV) for k, v in data.items()}, batch_idx=bidx)
        _check(d, out, dict(ref, batch_idx=[t.to(dtype) for t in ref['batch_idx']]), groups, 0.3, f'strided, {dtype}')
        assert out['batch_idx'][0].dtype == dtype
    # a batch_idx outside [0, B): the status word, reported at the one host read
    bad = data['batch_idx'].clone()
    bad[-1] = 3
    pend = GS.group_sample_launch(*(data[k].to(DEV) for k in ('seg_logits', 'vote_offsets', 'seg_points')), bad.to(DEV), groups, thr, 3)
    with pytest.raises(RuntimeError, match='batch_idx holds a value outside'):
        pend.finish()
    with pytest.raises(RuntimeError, match='non-decreasing'):
        GS.group_sample_launch(*(data[k].to(DEV) for k in ('seg_logits', 'vote_offsets', 'seg_points')),
                               data['batch_idx'].flip(0).to(DEV), groups, thr, 3, validate=True)
    # apply_rule=False leaves an empty group empty
    lg = data['seg_logits'].clone()
    lg[:, 9] = -30.0
    out = GS.group_sample(lg.to(DEV), data['vote_offsets'].to(DEV), data['seg_points'].to(DEV), data['batch_idx'].to(DEV), groups, thr,
                          3, apply_rule=False)
    assert out['totals'][3] == 0 and out['rule'] == [False] * 6


def test_one_host_read_per_stage():
    """the stage queues its launches without reading the device; finish() is the one read"""
    from sst_amd import fg_group_sample as GS
    data, groups, thr = _small(600, seed=7)
    d = {k: v.to(DEV) for k, v in data.items()}
    GS.group_sample(d['seg_logits'], d['vote_offsets'], d['seg_points'], d['batch_idx'], groups, thr, 2)     # library loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        pend = GS.group_sample_launch(d['seg_logits'], d['vote_offsets'], d['seg_points'], d['batch_idx'], groups, thr, 2)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    out = pend.finish()
    torch.cuda.set_sync_debug_mode('error')
    try:
        rows, _ = GS.virtual_rows(out, d['seg_feats'].requires_grad_(), d['seg_logits'], d['seg_points'], PC_RANGE)
        rows.sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert d['seg_feats'].grad is not None


@pytest.mark.parametrize('path', ['grouped', 'per_class'])
def test_virtual_rows_forward_and_backward(path):
    from sst_amd import fg_group_sample as GS
    from sst_amd import fg_sample as FS
    from sst_amd.virtual_voxel import VirtualVoxelExtractor
    if path == 'grouped':
        data, groups, thr = _small(700, b=3, seed=8)
        d = {k: v.to(DEV) for k, v in data.items()}
        out = GS.group_sample(d['seg_logits'], d['vote_offsets'], d['seg_points'], d['batch_idx'], groups, thr, 3, 0.3)
    else:                                                   # the Waymo path: per-class sigmoid scores, rows from fg_sample
        import fsd_sample_ref as R1
        data, thr = R1.make_case(700, 3, 3, 8, seed=9, p_cols=5)
        d = {k: v.to(DEV) for k, v in data.items()}
        d['seg_points'] = d['seg_points'] * torch.tensor([1., 1., 0.3, 1., 1.], device=DEV)
        out = FS.fg_sample(d['seg_logits'], d['vote_offsets'], d['seg_points'], d['batch_idx'], thr, 3)
    masks = torch.stack(out['fg_mask_list'])
    assert int(masks.sum(0).max()) >= 2, 'some point is a row of two groups: its gradient is a sum'
    feats = d['seg_feats'].clone().requires_grad_()
    rows, clipped = GS.virtual_rows(out, feats, d['seg_logits'], d['seg_points'], PC_RANGE)
    # the cat of extract_feat over the same rows, through boolean indexing
    ref_feats = d['seg_feats'].clone().requires_grad_()
    comb = {k: torch.cat([t[m] for m in masks]) for k, t in (('seg_feats', ref_feats), ('seg_logits', d['seg_logits']),
                                                             ('seg_points', d['seg_points']))}
    centers = VirtualVoxelExtractor.clip_points(None, torch.cat(out['center_preds']).clone(), PC_RANGE)
    offset = (centers - comb['seg_points'][:, :3]) / 10
    want = torch.cat([comb['seg_feats'], offset, comb['seg_logits'], comb['seg_points'][:, 3:]], 1)
    _bits(rows, want, 'virtual_input')
    _bits(clipped, centers, 'clipped centres')
    assert bool((centers != torch.cat(out['center_preds'])).any()), 'some centre is clipped'
    assert not clipped.requires_grad
    g = torch.Generator().manual_seed(3)
    d_out = torch.randint(-4, 5, tuple(rows.shape), generator=g).float().to(DEV)
    rows.backward(d_out)
    want.backward(d_out)
    _bits(feats.grad, ref_feats.grad, 'd seg_feats (integer-valued: every order of the sum is exact)')
    assert bool((feats.grad[~masks.any(0)] == 0).all()) and bool((feats.grad != 0).any())
    # real-valued gradients: the same bits in two runs
    d_real = torch.randn(tuple(rows.shape), generator=g).to(DEV)
    runs = []
    for _ in range(2):
        f2 = d['seg_feats'].clone().requires_grad_()
        GS.virtual_rows(out, f2, d['seg_logits'], d['seg_points'], PC_RANGE)[0].backward(d_real)
        runs.append(f2.grad)
    _bits(runs[0], runs[1], 'backward twice')
