"""The FSD foreground sampling stage restated in torch: boolean-mask indexing as the reference does it
(mmdet3d/models/detectors/single_stage_fsd.py:571-593, 698-797; two_stage_fsd.py:108-178), with a STABLE sort where the reference
calls ``Tensor.sort()``.  tests/test_fsd_sample_host.py pins these functions to tests/golden/fsd_sample.npz (the reference's own
methods executed from their source text) on the CPU; the GPU tests compare the kernels against them on the device.

It is also the data flow that existed before the kernels: tools/fg_sample_bench.py times it as the yardstick."""
import numpy as np
import torch

MARGIN = 1e-6          # a test logit's float64 sigmoid stays this far from its class's float32 threshold


def thresholds32(score_thresh, threshold_buffer=0.0):
    """``score_thresh[c] + buffer`` (Python double) rounded to float32 once, as torch rounds a Python scalar operand"""
    return [float(np.float32(float(t) + float(threshold_buffer))) for t in score_thresh]


def margin_ok(logits, thr32):
    """bool [N, C]: the float64 sigmoid of the logit is at least MARGIN away from the float32 threshold of its class"""
    p = torch.sigmoid(logits.double())
    t = torch.tensor([float(np.float32(x)) if np.isfinite(x) else 2.0 for x in thr32], dtype=torch.float64, device=logits.device)
    return (p - t[None]).abs() >= MARGIN


def redraw_until_clear(logits, thr32, generator=None):
    """replace every logit that is ambiguous against its threshold (see MARGIN); returns the logits, all of them clear"""
    logits = logits.clone()
    for _ in range(100):
        bad = ~margin_ok(logits, thr32)
        if not bad.any():
            return logits
        logits[bad] = (torch.randn(int(bad.sum()), generator=generator, dtype=torch.float64) * 2).to(logits.dtype).to(logits.device)
    raise AssertionError('could not draw unambiguous logits')


def first_positions(batch_idx):
    """get_sample_beg_position (:750-754): the first point of every sample that is present"""
    b = batch_idx.long()
    head = torch.ones_like(b, dtype=torch.bool)
    if b.numel() > 1:
        order = torch.argsort(b, stable=True)
        sb = b[order]
        is_head = torch.ones_like(sb, dtype=torch.bool)
        is_head[1:] = sb[1:] != sb[:-1]
        head = torch.zeros_like(is_head)
        head[order] = is_head
    return torch.where(head)[0]


def fg_masks(seg_logits, batch_idx, thr32, extra_mask=None):
    """get_fg_mask + the at-least-one rule of sample (:720-729) -> (masks bool [C, N], rule: list of bool)"""
    n, c = seg_logits.shape
    scores = seg_logits.sigmoid()
    batch_size = int(batch_idx.max().item()) + 1 if n else 0
    masks, rules = [], []
    for k in range(c):
        thr = thr32[k]
        m = scores[:, k] > thr if np.isfinite(thr) else torch.zeros(n, dtype=torch.bool, device=seg_logits.device)
        if extra_mask is not None:
            m = m | extra_mask[k]
        rule = len(torch.unique(batch_idx[m])) < batch_size
        if rule:
            m = m.clone()
            m[first_positions(batch_idx)] = True
        masks.append(m)
        rules.append(bool(rule))
    return (torch.stack(masks) if c else torch.zeros((0, n), dtype=torch.bool)), rules


def topk_extra_mask(seg_logits, topks):
    """the disable_pretrain branch of get_fg_mask (:757-763)"""
    n, c = seg_logits.shape
    scores = seg_logits.sigmoid()
    mask = torch.zeros((c, n), dtype=torch.bool, device=seg_logits.device)
    for k in range(c):
        mask[k, torch.topk(scores[:, k], min(int(topks[k]), n))[1]] = True
    return mask


def sample(data, thr32, extra_mask=None):
    """``sample`` (:698-748) over data = dict(seg_points, seg_logits, seg_vote_preds, seg_feats, batch_idx, vote_offsets): per-class
    lists of every entry + fg_mask_list + center_preds (+ rule)"""
    masks, rules = fg_masks(data['seg_logits'], data['batch_idx'], thr32, extra_mask)
    c = masks.size(0)
    offset = data['vote_offsets'].reshape(-1, c, 3)
    xyz = data['seg_points'][:, :3]
    out = {name: [t[m] for m in masks] for name, t in data.items()}
    out['fg_mask_list'] = list(masks)
    out['center_preds'] = [xyz[m] + offset[m, k] for k, m in enumerate(masks)]
    out['rule'] = rules
    return out


def update_by_mask(sampled, valid_mask_list):
    """update_sample_results_by_mask (:571-586)"""
    out = {}
    for name, old in sampled.items():
        if name == 'rule':
            continue
        if 'fg_mask' in name:
            new = []
            for data, mask in zip(old, valid_mask_list):
                d = data.clone()
                d[data] = mask
                new.append(d)
            out[name] = new
        else:
            out[name] = [d[m] for d, m in zip(old, valid_mask_list)]
    return out


def combine(sampled):
    """combine_classes + the column concatenation of forward_train (:529-532) -> dict(points, pts_feats, center_preds)"""
    cat = {k: torch.cat(sampled[k], 0) for k in ('seg_points', 'seg_logits', 'seg_vote_preds', 'seg_feats', 'center_preds')}
    return dict(points=cat['seg_points'], center_preds=cat['center_preds'],
                pts_feats=torch.cat([cat['seg_logits'], cat['seg_vote_preds'], cat['seg_feats']], 1))


def roi_multi(points, cluster_pts_feats, seg_feats, pts_mask, batch_idx):
    """prepare_multi_class_roi_input (two_stage_fsd.py:127-178) with a stable sort"""
    bg = sum(m.long() for m in pts_mask) == 0
    all_points = torch.cat([points[bg]] + [points[m] for m in pts_mask], 0)
    all_seg = torch.cat([seg_feats[bg]] + [seg_feats[m] for m in pts_mask], 0)
    pad = cluster_pts_feats.new_zeros(int(bg.sum()), cluster_pts_feats.shape[1])
    all_cluster = torch.cat([pad, cluster_pts_feats], 0)
    all_batch = torch.cat([batch_idx[bg]] + [batch_idx[m] for m in pts_mask], 0)
    cat_feats = torch.cat([all_cluster, all_seg], 1)
    all_batch, inds = all_batch.sort(stable=True)
    return all_points[inds], cat_feats[inds], all_batch


def roi_single(points, cluster_pts_feats, seg_feats, pts_mask, batch_idx):
    """prepare_roi_input (two_stage_fsd.py:108-125)"""
    pad = cluster_pts_feats.new_zeros(points.shape[0], cluster_pts_feats.shape[1])
    pad[pts_mask[0]] = cluster_pts_feats
    return points, torch.cat([pad, seg_feats], 1), batch_idx


def make_case(n, c, b, f, seed, p_cols=4, fg=0.3, empty_samples=(), int_feats=False, device='cpu'):
    """a synthetic batch: points sorted by sample (samples in ``empty_samples`` have no point), logits with about ``fg`` of the
    points over a threshold of 0.5 per class, every logit clear of it by MARGIN"""
    g = torch.Generator().manual_seed(seed)
    present = [s for s in range(b) if s not in empty_samples]
    bidx = torch.tensor(sorted(present[int(i)] for i in torch.randint(0, len(present), (n,), generator=g)), dtype=torch.int64) \
        if n else torch.zeros(0, dtype=torch.int64)
    shift = float(torch.distributions.Normal(0., 1.).icdf(torch.tensor(fg))) * 2
    logits = (torch.randn(n, c, generator=g, dtype=torch.float64) * 2 + shift).float()
    thr = thresholds32([0.5] * c)
    logits = redraw_until_clear(logits, thr, g)
    draw = (lambda *s: torch.randint(-8, 9, s, generator=g).float()) if int_feats else (lambda *s: torch.randn(*s, generator=g))
    data = dict(seg_points=torch.randn(n, p_cols, generator=g) * 10, seg_logits=logits, seg_vote_preds=draw(n, 3 * c),
                seg_feats=draw(n, f), batch_idx=bidx, vote_offsets=torch.randn(n, 3 * c, generator=g))
    return {k: v.to(device) for k, v in data.items()}, thr
