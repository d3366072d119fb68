"""Generates tests/golden/fsdv2_sample.npz: the FSDv2 grouped sampling stage as the REFERENCE computes it (data only).

Needs the reference tree (oracle.ref_loader); run from the repository root:  python tests/golden/make_fsdv2_sample.py

Executed from their source text on the CPU: SingleStageFSDV2.batched_group_sample / group_sample / get_fg_mask /
get_sample_beg_position / get_offset_weight / gather_group_by_names / combine_classes / clip_points
(detectors/single_stage_fsd_v2.py) and FSDV2.pre_voxelize (detectors/two_stage_fsd_v2.py).  What these import from compiled
extensions is stood in for, as tests/golden/make_fsd_sample.py does:
  get_inner_win_inds     oracle.ref_loader.stable_ingroup_rank (rank of every element inside its group, stable)
  scatter_v2 ('avg')     the mean of the rows of every group of the given inverse map (index_add / counts), -> (means, new_coors)
  Tensor.sort()          of FSDV2.forward_train (two_stage_fsd_v2.py:104): the STABLE sort (the reference leaves the order inside a
                         sample open; the library fixes the stable one)
The detector object is a plain record with the attributes the methods read.  The lines of extract_feat that form the projector
input (:172-176) and of FSDV2.forward_train that select and sort the second stage's points (:95-106) are statements inside long
methods; they are written out here next to the reference's clip_points / pre_voxelize.

Feature and vote-prediction values are small integers, the points multiples of 1/64 and, outside the cases ``nusc`` and ``scale``,
the vote offsets multiples of 1/64 (the file compresses); the logits are real.  Every logit row's float64 grouped scores are at
least (K + 8) * 2^-23 away from the float32 thresholds, and the reference's float32 masks equal those of its float64 run (both
asserted).  center_preds of ``nusc`` and ``tie3`` is recorded from the float64 run too; the full projector input of ``nusc`` only
(elsewhere its three computed columns)."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import fsdv2_sample_ref as R  # noqa: E402

SS_PY = 'mmdet3d/models/detectors/single_stage_fsd_v2.py'
TS_PY = 'mmdet3d/models/detectors/two_stage_fsd_v2.py'
PC_RANGE = [-51.2, -51.2, -5, 51.2, 51.2, 3]
FEATS = 8


class Cfg(dict):
    __getattr__ = dict.get


def scatter_avg(feat, coors, mode, return_inv=True, min_points=0, unq_inv=None, new_coors=None):
    assert mode == 'avg' and unq_inv is not None and new_coors is not None and min_points == 0
    return R.scatter_avg(feat, unq_inv, new_coors.size(0)), new_coors


def reference_parts():
    from oracle import ref_loader
    glb = {'get_inner_win_inds': ref_loader.stable_ingroup_rank, 'scatter_v2': scatter_avg}
    parts = {name: ref_loader.load_reference_method(SS_PY, 'SingleStageFSDV2', name, glb)
             for name in ('batched_group_sample', 'group_sample', 'get_fg_mask', 'get_sample_beg_position', 'get_offset_weight',
                          'gather_group_by_names', 'combine_classes', 'clip_points')}
    parts['pre_voxelize'] = ref_loader.load_reference_method(TS_PY, 'FSDV2', 'pre_voxelize', glb)
    return parts


def detector(parts, num_classes, cfg, training, runtime_info=None):
    det = types.SimpleNamespace(num_classes=num_classes, cfg=cfg, train_cfg=cfg, test_cfg=cfg, training=training,
                                runtime_info=runtime_info if runtime_info is not None else {}, pc_range=PC_RANGE)
    for name, fn in parts.items():
        setattr(det, name, types.MethodType(fn, det))
    return det


def run_case(out, parts, name, data, class_names, group_names, score_thresh, offset_scale=None, training=False, runtime_info=None,
             topks=None, batched=True):
    k = data['seg_logits'].size(1)
    cfg = dict(score_thresh=score_thresh, class_names=class_names, group_names=group_names, offset_weight='max')
    cfg['batched_group_sample' if batched else 'group_sample'] = True
    if offset_scale is not None:
        cfg['offset_scale'] = offset_scale
    if topks is not None:
        cfg.update(disable_pretrain=True, disable_pretrain_topks=topks)
    det = detector(parts, k - 1, Cfg(cfg), training, runtime_info)
    groups = R.groups_by_names(group_names, class_names)
    topk = training and topks is not None and not (runtime_info or {}).get('enable_detection', False)
    buf = (runtime_info or {}).get('threshold_buffer', 0) if training else 0
    thr = [float('inf')] * len(groups) if topk else R.thresholds32(score_thresh, buf)
    assert bool(R.margin_ok(data['seg_logits'], groups, thr).all()), name
    batch = int(data['batch_idx'].max()) + 1
    run = det.batched_group_sample if batched else det.group_sample
    smp = run(dict(data), data['vote_offsets'])
    d64 = {key: (v.double() if v.is_floating_point() else v) for key, v in data.items()}
    smp64 = run(dict(d64), d64['vote_offsets'])
    scores = det.gather_group_by_names(data['seg_logits'].softmax(1)[:, :-1])
    pre = [det.get_fg_mask(scores, None, g, None, None, None) for g in range(len(groups))]
    if batched:
        rule = [len(torch.unique(data['batch_idx'][m])) < batch for m in pre]
    else:
        rule = [not bool(m.any()) for m in pre]
    for key in R.KEYS:
        out[f'{name}_{key}'] = data[key].numpy()
    out[f'{name}_thr32'] = np.array(thr, dtype=np.float64)
    out[f'{name}_batch'] = np.int64(batch)
    out[f'{name}_batched'] = np.bool_(batched)
    out[f'{name}_offset_scale'] = np.float64(1 if offset_scale is None else offset_scale)
    out[f'{name}_rule'] = np.array(rule)
    out[f'{name}_group_len'] = np.array([len(g) for g in groups])
    out[f'{name}_group_class'] = np.array([c for g in groups for c in g])
    if topk:
        out[f'{name}_extra'] = torch.stack(pre).numpy()
        out[f'{name}_topks'] = np.array(topks)
    for g in range(len(groups)):
        assert torch.equal(smp['fg_mask_list'][g], smp64['fg_mask_list'][g]), (name, g)
        for key in ('seg_points', 'batch_idx', 'center_preds'):
            out[f'{name}_s_{key}_{g}'] = smp[key][g].numpy()
        if name in ('nusc', 'tie3'):
            out[f'{name}_s_center_preds_f64_{g}'] = smp64['center_preds'][g].numpy()
        out[f'{name}_s_fg_mask_{g}'] = smp['fg_mask_list'][g].numpy()
    comb = det.combine_classes(smp, ['seg_points', 'seg_logits', 'seg_vote_preds', 'seg_feats', 'center_preds', 'batch_idx'])
    centers = det.clip_points(comb['center_preds'].clone(), PC_RANGE)
    offset = (centers - comb['seg_points'][:, :3]) / 10                                     # extract_feat :175-176
    if name == 'nusc':                   # the other columns are copies of rows: once is enough
        out[f'{name}_virtual_input'] = torch.cat([comb['seg_feats'], offset, comb['seg_logits'], comb['seg_points'][:, 3:]], 1).numpy()
    out[f'{name}_virtual_offset'] = offset.numpy()
    out[f'{name}_clipped'] = centers.numpy()
    out[f'{name}_c_batch_idx'] = comb['batch_idx'].numpy()
    print(f'{name}: N {data["seg_points"].size(0)}, K {k}, selected {[int(m.sum()) for m in smp["fg_mask_list"]]}, rule {rule}, '
          f'clipped {int((centers != comb["center_preds"]).any(1).sum())} of {centers.size(0)}')
    return smp


def case_data(n, k, b, seed, groups, thr, fg=0.2, coarse_votes=True):
    data = R.make_case(n, k, b, FEATS, seed, groups, thr, fg=fg)
    if coarse_votes:
        data['vote_offsets'] = (torch.round(data['vote_offsets'] * 64) / 64).clamp(-2, 2)
    data['seg_vote_preds'] = data['seg_vote_preds'].clamp(-1, 1)      # only ever copied
    return data


def set_rows(data, rows, group, value, groups):
    """the logits of ``rows``: ``value`` on every class of ``group`` (a tie when the group has several), -4 on the other classes and
    0 on the background"""
    data['seg_logits'][rows] = -4.0
    data['seg_logits'][rows, -1] = 0.0
    for c in groups[group]:
        data['seg_logits'][rows, c] = value


def main():
    parts = reference_parts()
    out, names = {}, []

    def add(name, *a, **kw):
        names.append(name)
        return run_case(out, parts, name, *a, **kw)

    cn, gn, st = R.NUSC_CLASSES, R.NUSC_GROUPS, R.NUSC_THRESH
    groups = R.groups_by_names(gn, cn)
    thr = R.thresholds32(st)
    add('nusc', case_data(400, 11, 2, 1, groups, thr, coarse_votes=False), cn, gn, st)

    # group 3 (barrier) empty in the middle sample; group 0 lacks sample 1 too but holds the first point of sample 0 already
    data = case_data(330, 11, 3, 2, groups, thr, fg=0.3)
    first = [int(torch.nonzero(data['batch_idx'] == s)[0, 0]) for s in range(3)]
    mid = torch.nonzero(data['batch_idx'] == 1)[:, 0]
    data['seg_logits'][mid, 9] = -9.0
    data['seg_logits'][mid, 0] = -9.0
    set_rows(data, [first[0]], 0, 3.0, groups)
    data['seg_logits'] = R.redraw_until_clear(data['seg_logits'], groups, thr, torch.Generator().manual_seed(22),
                                              keep=(data['batch_idx'] == 1) | (torch.arange(330) == first[0]))
    data['seg_logits'][mid, 9] = -9.0
    data['seg_logits'][mid, 0] = -9.0
    smp = add('rule_pair', data, cn, gn, st)
    assert out['rule_pair_rule'][3] and out['rule_pair_rule'][0] and int((data['batch_idx'][smp['fg_mask_list'][3]] == 1).sum()) == 1

    # exact two-way ties of a group's logits in rows that are selected (and in some that are not)
    data = case_data(300, 11, 2, 3, groups, thr)
    g = torch.Generator().manual_seed(33)
    rows = torch.randperm(300, generator=g)[:60]
    for j, grp in enumerate((1, 2, 4, 5)):
        set_rows(data, rows[15 * j:15 * j + 10], grp, 1.5, groups)
        for c in groups[grp]:
            data['seg_logits'][rows[15 * j + 10:15 * j + 15], c] = -2.5
    data['seg_logits'] = R.redraw_until_clear(data['seg_logits'], groups, thr, g)
    add('tie2', data, cn, gn, st)

    # an Argoverse-like K = 27 with three-class groups tied
    cn3 = [f'c{i}' for i in range(26)]
    gn3 = [['c0'], ['c3', 'c1', 'c2'], ['c4', 'c5', 'c6', 'c7'], ['c8', 'c9', 'c10'], ['c11', 'c25', 'c12', 'c13', 'c14'],
           ['c15', 'c16', 'c17', 'c18', 'c19', 'c20', 'c21', 'c22', 'c23', 'c24']]
    st3 = [0.4, 0.25, 0.25, 0.25, 0.25, 0.25]
    groups3, thr3 = R.groups_by_names(gn3, cn3), R.thresholds32(st3)
    data = case_data(300, 27, 2, 4, groups3, thr3)
    rows = torch.randperm(300, generator=g)[:40]
    set_rows(data, rows[:15], 1, 2.0, groups3)
    set_rows(data, rows[15:30], 3, 1.0, groups3)
    set_rows(data, rows[30:40], 2, 1.0, groups3)                                            # a four-way tie
    data['seg_logits'][rows[30:40], 7] = -4.0                                               # ... made three-way
    data['seg_logits'] = R.redraw_until_clear(data['seg_logits'], groups3, thr3, g)
    add('tie3', data, cn3, gn3, st3)

    # a logit 5e-7 below the maximum counts as a tie, one 2e-6 below does not
    data = case_data(300, 11, 2, 5, groups, thr)
    rows = torch.randperm(300, generator=g)[:40]
    for j, grp in enumerate((1, 2, 4, 5)):
        set_rows(data, rows[10 * j:10 * j + 10], grp, 2.0, groups)
        data['seg_logits'][rows[10 * j:10 * j + 5], groups[grp][1]] = 2.0 - 5e-7
        data['seg_logits'][rows[10 * j + 5:10 * j + 10], groups[grp][0]] = 2.0 - 2e-6
    lg = data['seg_logits'][rows[:5]][:, groups[1]]
    assert bool(((lg - lg.max(1)[0][:, None]).abs() < 1e-6).all()) and bool((lg[:, 0] != lg[:, 1]).all())
    lg = data['seg_logits'][rows[5:10]][:, groups[1]]
    assert int(((lg - lg.max(1)[0][:, None]).abs() < 1e-6).sum()) == 5
    data['seg_logits'] = R.redraw_until_clear(data['seg_logits'], groups, thr, g)
    add('near_tie', data, cn, gn, st)

    add('scale', case_data(300, 11, 2, 6, groups, thr, coarse_votes=False), cn, gn, st, offset_scale=0.3)

    info = dict(threshold_buffer=0.05, enable_detection=True)
    thr_b = R.thresholds32(st, 0.05)
    add('buffer', case_data(300, 11, 2, 7, groups, thr_b), cn, gn, st, training=True, runtime_info=info,
        topks=[500] * 10)

    data = case_data(300, 11, 2, 8, groups, [float('inf')] * 6)
    add('topk', data, cn, gn, st, training=True, runtime_info={}, topks=[40, 20, 400, 10, 5, 1, 500, 500, 500, 500])
    sc = R.grouped_scores(data['seg_logits'], groups)
    assert all(len(torch.unique(sc[:, j])) == 300 for j in range(6)), 'topk: the grouped scores must be distinct'
    for j, kk in enumerate([40, 20, 400, 10, 5, 1]):        # the last score taken and the first one left are far apart: any softmax agrees
        top = torch.sort(sc[:, j].double(), descending=True)[0]
        assert kk >= 300 or float((top[kk - 1] - top[kk]) / top[kk - 1]) > 1e-4, ('topk', j)

    gn_u = [['car'], ['truck', 'construction_vehicle'], ['barrier'], ['pedestrian', 'traffic_cone']]   # bus, trailer, cycles: no group
    st_u = [0.2, 0.2, 0.1, 0.1]
    groups_u, thr_u = R.groups_by_names(gn_u, cn), R.thresholds32(st_u)
    add('unlisted', case_data(300, 11, 2, 9, groups_u, thr_u), cn, gn_u, st_u)

    gn_1 = [['pedestrian', 'car', 'bicycle']]
    groups_1, thr_1 = R.groups_by_names(gn_1, cn), R.thresholds32([0.3])
    add('one_group', case_data(350, 11, 2, 10, groups_1, thr_1), cn, gn_1, [0.3])

    data = case_data(300, 11, 1, 11, groups, thr)
    data['seg_logits'][:, 9] = -9.0                                                         # barrier selects nothing
    data['seg_logits'] = R.redraw_until_clear(data['seg_logits'], groups, thr, g)
    data['seg_logits'][:, 9] = -9.0
    assert bool(R.margin_ok(data['seg_logits'], groups, thr).all())
    add('unbatched', data, cn, gn, st, batched=False)
    assert out['unbatched_rule'][3] and out['unbatched_s_fg_mask_3'].sum() == 1
    out['cases'] = np.array(names)

    # second stage: the rows extract_feat hands on (original points, then the voted centres), 0.5 m voxels or none
    g = torch.Generator().manual_seed(12)
    n_ori, n_vir = 260, 90
    xyz = torch.round((torch.rand(n_ori + n_vir, 3, generator=g) * torch.tensor([8., 8., 3.]) - torch.tensor([4., 4., 2.])) * 64) / 64
    feats = torch.randint(-8, 9, (n_ori + n_vir, 6), generator=g).float()
    bidx = torch.cat([torch.sort(torch.randint(0, 2, (n_ori,), generator=g))[0], torch.sort(torch.randint(0, 2, (n_vir,), generator=g))[0]])
    ind = torch.cat([torch.zeros(n_ori), torch.ones(n_vir)])
    out['ss_pts_xyz'], out['ss_pts_feats'], out['ss_pts_batch_inds'], out['ss_pts_indicators'] = (t.numpy() for t in (xyz, feats, bidx, ind))
    out['ss_pc_range'] = np.array(PC_RANGE, dtype=np.float64)
    out['ss_voxel_size'] = np.array([0.5, 0.5, 0.5])
    for with_virtual in (False, True):
        for voxel in (None, (0.5, 0.5, 0.5)):
            det = detector(parts, 10, Cfg(dict(pre_2nd_voxelization=voxel)), False)
            a, b, c = xyz, feats, bidx
            if not with_virtual:                                                            # two_stage_fsd_v2.py:95-99
                ori = ind == 0
                a, b, c = a[ori], b[ori], c[ori]
            a, b, c = det.pre_voxelize(a, b, c)
            c, inds = torch.sort(c, stable=True)                                            # :104, stable
            a, b = a[inds], b[inds]
            tag = f'ss_v{int(with_virtual)}_p{int(voxel is not None)}'
            out[f'{tag}_xyz'], out[f'{tag}_feats'], out[f'{tag}_batch'] = a.numpy(), b.numpy(), c.numpy()
            print(f'{tag}: {xyz.size(0)} rows -> {a.size(0)}')

    out = {key: np.asfortranarray(v) if isinstance(v, np.ndarray) and v.ndim == 2 else v for key, v in out.items()}
    path = os.path.join(ROOT, 'tests', 'golden', 'fsdv2_sample.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays')


if __name__ == '__main__':
    main()
