"""The FSDv2 grouped sampling stage restated in torch: boolean-mask indexing as the reference does it
(mmdet3d/models/detectors/single_stage_fsd_v2.py:124-129, 164-176, 656-705, 726-891; two_stage_fsd_v2.py:95-106, 172-199), with a
STABLE sort where the reference calls ``Tensor.sort()``.  tests/test_fsdv2_sample_host.py pins these functions to
tests/golden/fsdv2_sample.npz (the reference's own methods executed from their source text) on the CPU; the GPU tests compare the
kernels against them on the device.

It is also the data flow that existed before the kernels: tools/fg_group_sample_bench.py times it as the yardstick."""
import numpy as np
import torch

from fsd_sample_ref import first_positions, thresholds32  # noqa: F401

NUSC_CLASSES = ['car', 'truck', 'trailer', 'bus', 'construction_vehicle', 'bicycle', 'motorcycle', 'pedestrian', 'traffic_cone',
                'barrier']
NUSC_GROUPS = [['car'], ['truck', 'construction_vehicle'], ['bus', 'trailer'], ['barrier'], ['motorcycle', 'bicycle'],
               ['pedestrian', 'traffic_cone']]
NUSC_THRESH = [0.2, 0.2, 0.2, 0.1, 0.1, 0.1]
KEYS = ('seg_points', 'seg_logits', 'seg_vote_preds', 'seg_feats', 'batch_idx', 'vote_offsets')

CASES = ['nusc', 'rule_pair', 'tie2', 'tie3', 'near_tie', 'scale', 'buffer', 'topk', 'unlisted', 'one_group', 'unbatched']


def case_of(gold, name):
    """a case of tests/golden/fsdv2_sample.npz -> (data, groups, thr32, extra mask or None, offset_scale, batched)"""
    _t = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # the file stores its matrices column-major
    data = {k: _t(gold[f'{name}_{k}']) for k in KEYS}
    lens, flat = [int(x) for x in gold[f'{name}_group_len']], [int(x) for x in gold[f'{name}_group_class']]
    groups, pos = [], 0
    for n in lens:
        groups.append(flat[pos:pos + n])
        pos += n
    thr = [float(x) for x in gold[f'{name}_thr32']]
    extra = _t(gold[f'{name}_extra']) if f'{name}_extra' in gold else None
    return data, groups, thr, extra, float(gold[f'{name}_offset_scale']), bool(gold[f'{name}_batched'])


def margin(num_logits):
    """a test logit's float64 grouped score stays this far from its group's float32 threshold: an fp32 softmax group sum has at
    most K + 3 roundings of quantities <= 1"""
    return (num_logits + 8) * 2.0 ** -23


def groups_by_names(group_names, class_names):
    return [[list(class_names).index(name) for name in names] for names in group_names]


def grouped_scores(seg_logits, groups):
    """``seg_logits.softmax(1)`` and gather_group_by_names (:879-891) -> [N, G] (in the dtype of the logits)"""
    scores = seg_logits.softmax(1)
    return torch.stack([scores[:, list(grp)].sum(1) for grp in groups], dim=1)


def margin_ok(seg_logits, groups, thr32):
    """bool [N, G]: the float64 grouped score is at least margin(K) away from the float32 threshold of its group"""
    s = grouped_scores(seg_logits.double(), groups)
    t = torch.tensor([float(np.float32(x)) if np.isfinite(x) else 2.0 for x in thr32], dtype=torch.float64, device=seg_logits.device)
    return (s - t[None]).abs() >= margin(seg_logits.size(1))


def redraw_until_clear(seg_logits, groups, thr32, generator=None, keep=None):
    """replace the rows that hold an ambiguous grouped score (rows in the bool mask ``keep`` must be clear as they are)"""
    logits = seg_logits.clone()
    for _ in range(100):
        bad = ~margin_ok(logits, groups, thr32).all(1)
        if not bad.any():
            return logits
        assert keep is None or not bool((bad & keep).any()), 'a hand-set row is ambiguous'
        logits[bad] = (torch.randn(int(bad.sum()), logits.size(1), generator=generator, dtype=torch.float64) * 2).to(logits.dtype)
    raise AssertionError('could not draw unambiguous logits')


def group_masks(seg_logits, batch_idx, groups, thr32, extra_mask=None, batched=True):
    """get_fg_mask on the grouped scores + the at-least-one rule (:816-824 batched, :752-759 not) -> (masks [G, N], rule list)"""
    n = seg_logits.size(0)
    scores = grouped_scores(seg_logits, groups)
    batch_size = int(batch_idx.max().item()) + 1 if n else 0
    masks, rules = [], []
    for g in range(len(groups)):
        thr = thr32[g]
        m = scores[:, g] > thr if np.isfinite(thr) else torch.zeros(n, dtype=torch.bool, device=seg_logits.device)
        if extra_mask is not None:
            m = m | extra_mask[g]
        if batched:
            rule = len(torch.unique(batch_idx[m])) < batch_size
            if rule:
                m = m.clone()
                m[first_positions(batch_idx)] = True
        else:
            rule = n > 0 and not bool(m.any())
            if rule:
                m = m.clone()
                m[0] = True
        masks.append(m)
        rules.append(bool(rule))
    return torch.stack(masks), rules


def topk_extra_mask(seg_logits, groups, topks):
    """the disable_pretrain branch of get_fg_mask (:663-669) on the grouped scores"""
    n = seg_logits.size(0)
    scores = grouped_scores(seg_logits, groups)
    mask = torch.zeros((len(groups), n), dtype=torch.bool, device=seg_logits.device)
    for g in range(len(groups)):
        mask[g, torch.topk(scores[:, g], min(int(topks[g]), n))[1]] = True
    return mask


def offset_weight(logits):
    """get_offset_weight, mode 'max' (:855-861)"""
    weight = ((logits - logits.max(1)[0][:, None]).abs() < 1e-6).to(logits.dtype)
    return weight / weight.sum(1)[:, None]


def group_sample(data, groups, thr32, offset_scale=1, extra_mask=None, batched=True):
    """``batched_group_sample`` (:790-853) / ``group_sample`` (:726-788, ``batched=False``: no offset scale) over
    data = dict(seg_points, seg_logits, seg_vote_preds, seg_feats, batch_idx, vote_offsets): per-group lists of every entry +
    fg_mask_list + center_preds (+ rule)"""
    logits = data['seg_logits']
    masks, rules = group_masks(logits, data['batch_idx'], groups, thr32, extra_mask, batched)
    offset = data['vote_offsets'].reshape(-1, logits.size(1), 3)
    xyz = data['seg_points'][:, :3]
    out = {name: [t[m] for m in masks] for name, t in data.items()}
    centers = []
    for grp, m in zip(groups, masks):
        this_offset = offset[:, list(grp), :][m]
        weight = offset_weight(logits[:, list(grp)][m])
        this_offset = (this_offset * weight[:, :, None]).sum(dim=1)
        centers.append(xyz[m] + offset_scale * this_offset if batched else xyz[m] + this_offset)
    out['fg_mask_list'] = list(masks)
    out['center_preds'] = centers
    out['rule'] = rules
    return out


def centers_f64(data, groups, masks, offset_scale=1):
    """the voted centres evaluated in float64 on the float32 inputs (the float32 scale, the float32 1e-6), and the bound of
    seven float32 roundings of quantities no larger than |p| + |scale| * sum |o_k|: -> (centres, bounds) lists per group"""
    logits = data['seg_logits']
    offset = data['vote_offsets'].reshape(-1, logits.size(1), 3).double()
    xyz, scale = data['seg_points'][:, :3].double(), float(np.float32(offset_scale))
    cen, bound, ties = [], [], []
    for grp, m in zip(groups, masks):
        lg = logits[:, list(grp)][m]
        tie = (lg - lg.max(1)[0][:, None]).abs() < 1e-6           # float32, as the kernel decides it
        w = tie.double() / tie.double().sum(1)[:, None]
        o = offset[:, list(grp), :][m]
        cen.append(xyz[m] + scale * (o * w[:, :, None]).sum(1))
        bound.append(8 * 2.0 ** -24 * (xyz[m].abs() + abs(scale) * (o.abs() * tie[:, :, None]).sum(1)))
        ties.append(tie.sum(1))
    return cen, bound, ties


def combine(sampled, names=('seg_points', 'seg_logits', 'seg_vote_preds', 'seg_feats', 'center_preds', 'batch_idx')):
    """combine_classes (:508-513)"""
    return {name: torch.cat(sampled[name], 0) for name in sampled if name in names}


def clip_bounds(pc_range, eps=1e-5):
    """the bounds as ``VirtualVoxelExtractor.clip_points`` forms them: float32 range +- eps in float32 arithmetic"""
    r = torch.tensor([float(v) for v in pc_range], dtype=torch.float32)
    return r[:3] + eps, r[3:] - eps


def virtual_input(combined, pc_range):
    """the projector input of extract_feat (:172-176) -> (rows, clipped centres).  ``/ 10`` is torch's own: a division on the CPU
    (what the golden holds), a product with the float32 reciprocal on a device tensor (what extract_feat computes there)"""
    lo, hi = clip_bounds(pc_range)
    pts = combined['seg_points']
    centers = torch.minimum(torch.maximum(combined['center_preds'], lo.to(pts.device)[None]), hi.to(pts.device)[None])
    offset = (centers - pts[:, :3]) / 10
    return torch.cat([combined['seg_feats'], offset, combined['seg_logits'], pts[:, 3:]], 1), centers


def scatter_avg(feat, inv, m):
    """the mean of the rows of every group of the inverse map (index_add / counts): the stand-in of scatter_v2(..., 'avg')"""
    out = torch.zeros((m, feat.size(1)), dtype=feat.dtype, device=feat.device).index_add_(0, inv, feat)
    cnt = torch.zeros(m, dtype=feat.dtype, device=feat.device).index_add_(0, inv, torch.ones(feat.size(0), dtype=feat.dtype, device=feat.device))
    return out / cnt[:, None]


def second_stage_input(pts_xyz, pts_feats, pts_batch_inds, pts_indicators, with_virtual, voxel_size, pc_range):
    """two_stage_fsd_v2.py:95-106 with FSDV2.pre_voxelize (:172-199): the original points (``with_virtual`` False), voxel means
    when ``voxel_size`` is given, then the stable sort by sample -> (xyz, feats, batch_inds)"""
    if not with_virtual:
        ori = pts_indicators == 0
        pts_xyz, pts_feats, pts_batch_inds = pts_xyz[ori], pts_feats[ori], pts_batch_inds[ori]
    if voxel_size is not None:
        vs = torch.tensor(voxel_size, dtype=pts_xyz.dtype, device=pts_xyz.device)
        lo = torch.tensor(pc_range[:3], dtype=pts_xyz.dtype, device=pts_xyz.device)
        coors = torch.div(pts_xyz[:, :3] - lo[None], vs[None], rounding_mode='floor').long()[:, [2, 1, 0]]
        coors = torch.cat([pts_batch_inds[:, None], coors], 1)
        new_coors, inv = torch.unique(coors, return_inverse=True, dim=0)
        pts_xyz, pts_feats = scatter_avg(pts_xyz, inv, new_coors.size(0)), scatter_avg(pts_feats, inv, new_coors.size(0))
        pts_batch_inds = new_coors[:, 0]
    pts_batch_inds, inds = torch.sort(pts_batch_inds, stable=True)
    return pts_xyz[inds], pts_feats[inds], pts_batch_inds


def make_case(n, k, b, f, seed, groups, thr32, p_cols=5, fg=0.2, int_feats=True, device='cpu'):
    """a synthetic batch: points sorted by sample, K = C + 1 logits with the background favoured so that about ``fg`` of the points
    pass some group, every grouped score clear of its threshold by margin(K)"""
    g = torch.Generator().manual_seed(seed)
    bidx = torch.sort(torch.randint(0, b, (n,), generator=g))[0] if n else torch.zeros(0, dtype=torch.int64)
    logits = (torch.randn(n, k, generator=g, dtype=torch.float64) * 2).float()
    logits[:, -1] += float(torch.distributions.Normal(0., 1.).icdf(torch.tensor(1.0 - fg))) * 2 + 2.0
    logits = redraw_until_clear(logits, groups, thr32, g)
    draw = (lambda *s: torch.randint(-8, 9, s, generator=g).float()) if int_feats else (lambda *s: torch.randn(*s, generator=g))
    pts = torch.randn(n, p_cols, generator=g) * 10
    data = dict(seg_points=torch.round(pts * 64) / 64, seg_logits=logits, seg_vote_preds=draw(n, 3 * k), seg_feats=draw(n, f).clamp(-1, 1),
                batch_idx=bidx, vote_offsets=torch.randn(n, 3 * k, generator=g))
    return {name: v.to(device) for name, v in data.items()}
