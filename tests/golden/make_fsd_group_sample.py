"""Generates tests/golden/fsd_group_sample.npz: the grouped foreground sampling of the FSD detectors as the REFERENCE computes
it (data only).

Needs the reference tree (oracle.ref_loader); run from the repository root:  python tests/golden/make_fsd_group_sample.py

Executed from their source text on the CPU (mmdet3d/models/detectors/single_stage_fsd.py): SingleStageFSD.group_sample,
gather_group_by_names, get_offset_weight, get_fg_mask and get_sample_beg_position.  Stood in for, as in make_fsd_sample.py:
  get_inner_win_inds     oracle.ref_loader.stable_ingroup_rank (rank of every element inside its group, stable)
The detector object is a plain record with the attributes the methods read (cfg / train_cfg / test_cfg, training,
runtime_info, num_classes).  Inputs (tests/fsd_group_sample_ref.make_case): 27 logits in Argoverse 2's six groups and 4 logits
in 2 groups, B = 1, 2, 3, a (group, sample) without any foreground so that the rule fires, rows with two equal maxima inside a
group.  Every grouped float64 score is at least (K + 8) * 2^-23 >= 1e-6 from its float32 threshold: ambiguous rows are redrawn
and the generator asserts that none is left - nothing is filtered silently."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import fsd_group_sample_ref as R  # noqa: E402

SS_PY = 'mmdet3d/models/detectors/single_stage_fsd.py'
METHODS = ('group_sample', 'gather_group_by_names', 'get_offset_weight', 'get_fg_mask', 'get_sample_beg_position')


class Cfg(dict):
    __getattr__ = dict.get


def reference_detector(num_classes, cfg, training=False, runtime_info=None):
    from oracle import ref_loader
    glb = {'get_inner_win_inds': ref_loader.stable_ingroup_rank}
    det = types.SimpleNamespace(num_classes=num_classes, cfg=cfg, train_cfg=cfg, test_cfg=cfg, training=training,
                                runtime_info=runtime_info if runtime_info is not None else {})
    for name in METHODS:
        setattr(det, name, types.MethodType(ref_loader.load_reference_method(SS_PY, 'SingleStageFSD', name, glb), det))
    return det


def run_case(out, name, layout, data, training=False, runtime_info=None, extra_cfg=None):
    classes, group_names, groups, _ = R.layout(layout)
    cfg = Cfg(dict(score_thresh=R.LAYOUTS[layout][2], group_names=group_names, class_names=classes, group_sample=True,
                   offset_weight='max', **(extra_cfg or {})))
    buf = (runtime_info or {}).get('threshold_buffer', 0) if training else 0
    topk = training and cfg.get('disable_pretrain', False) and not (runtime_info or {}).get('enable_detection', False)
    thr = [float('inf')] * len(groups) if topk else R.thresholds32(cfg['score_thresh'], buf)
    assert bool(R.margin_ok(data['seg_logits'], groups, thr).all()), f'{name}: a grouped score is ambiguous'
    assert float(R.V.margin(len(classes) + 1)) >= 1e-6
    det = reference_detector(len(classes), cfg, training, runtime_info)
    smp = det.group_sample(dict(data), data['vote_offsets'])
    scores = det.gather_group_by_names(data['seg_logits'].softmax(1)[:, :-1])
    bsz = int(data['batch_idx'].max()) + 1
    rule = []
    for g in range(len(groups)):
        pre = det.get_fg_mask(scores, None, g, None, None, None)
        rule.append(len(torch.unique(data['batch_idx'][pre])) < bsz)
    for k in R.KEYS:
        out[f'{name}_{k}'] = data[k].numpy()
    out[f'{name}_layout'] = np.array(layout)
    out[f'{name}_thr32'] = np.array(thr, dtype=np.float64)
    out[f'{name}_batch'] = np.int64(bsz)
    out[f'{name}_rule'] = np.array(rule)
    out[f'{name}_grouped_scores'] = scores.numpy()
    if topk:
        out[f'{name}_topks'] = np.array(cfg['disable_pretrain_topks'])
    for g in range(len(groups)):
        for key in ('seg_points', 'batch_idx', 'center_preds'):
            out[f'{name}_s_{key}_{g}'] = smp[key][g].numpy()
        out[f'{name}_s_fg_mask_{g}'] = smp['fg_mask_list'][g].numpy()
        w = det.get_offset_weight(data['seg_logits'][:, groups[g]][smp['fg_mask_list'][g]])
        out[f'{name}_s_weight_{g}'] = w.numpy()
    print(f'{name}: N {data["seg_points"].size(0)}, B {bsz}, selected {[int(m.sum()) for m in smp["fg_mask_list"]]}, rule {rule}')


def main():
    out, names = {}, []

    def add(name, *a, **kw):
        names.append(name)
        run_case(out, name, *a, **kw)

    for layout in ('argo2', 'small'):
        _, _, groups, thr = R.layout(layout)
        n = 140 if layout == 'argo2' else 300          # 81 vote columns per row: the file stays under the size limit
        for b in (1, 2, 3):
            add(f'{layout}_b{b}', layout, R.make_case(n, layout, b, seed=10 * b + len(layout)))
        # a (group, sample) without any foreground: the last group's classes far below in sample 0 -> the rule fires there
        data = R.make_case(n + 20, layout, 3, seed=41)
        lg = data['seg_logits'].clone()
        lg[(data['batch_idx'] == 0)[:, None] & torch.zeros_like(lg, dtype=torch.bool).index_fill_(1, torch.tensor(groups[-1]), True)] = -30.0
        data['seg_logits'] = lg
        add(f'{layout}_rule', layout, data)
        # every group empty in sample 1
        data = R.make_case(n + 20, layout, 2, seed=42)
        lg = data['seg_logits'].clone()
        lg[data['batch_idx'] == 1, :-1] = -30.0
        data['seg_logits'] = lg
        add(f'{layout}_rule_all', layout, data)
        # two equal maxima inside a group, in every fourth row
        data = R.make_case(n, layout, 2, seed=43)
        add(f'{layout}_tie2', layout, R.with_equal_maxima(data, groups, thr, torch.arange(0, n, 4)))
        thr_b = R.layout(layout, 0.1)[3]
        add(f'{layout}_buffer', layout, R.make_case(n, layout, 2, seed=44, threshold_buffer=0.1), training=True,
            runtime_info=dict(threshold_buffer=0.1, enable_detection=True))
        assert thr_b != thr
        data = R.make_case(n, layout, 2, seed=45)
        add(f'{layout}_topk', layout, data, training=True, runtime_info={},
            extra_cfg=dict(disable_pretrain=True, disable_pretrain_topks=[40, 7, n, 20, 1, 5][:len(groups)]))
    out['cases'] = np.array(names)
    out = {k: np.asfortranarray(v) if isinstance(v, np.ndarray) and v.ndim == 2 else v for k, v in out.items()}
    path = os.path.join(ROOT, 'tests', 'golden', 'fsd_group_sample.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays')
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
