"""``SingleStageFSD.group_sample`` (mmdet3d/models/detectors/single_stage_fsd.py:818-919) restated with plain torch operations,
for the tests of the grouped sampling path of the FSD detectors.  Test helper: torch only, any device.

The arithmetic is the one FSDv2's ``batched_group_sample`` has with ``offset_scale = 1`` (tests/fsdv2_sample_ref.py, whose
building blocks are used): fp32 softmax over ``num_classes + 1`` logits, the scores of a group's classes summed (background
excluded), ``score > thr`` per group, a point per sample wherever a group has a sample without any (the first point of every
sample), and the centre ``point + sum_k w_k offset_k`` with ``get_offset_weight``'s 'max' weights (maxima within 1e-6 share).
With one or two maxima the weights are 1 or 0.5 and the products exact, so the centre is the same bits however it is summed."""
import torch

import fsd_sample_ref as S
import fsdv2_sample_ref as V

KEYS = V.KEYS
ARGO2_CLASSES = ['Regular_vehicle', 'Pedestrian', 'Bicyclist', 'Motorcyclist', 'Wheeled_rider', 'Bollard', 'Construction_cone',
                 'Sign', 'Construction_barrel', 'Stop_sign', 'Mobile_pedestrian_crossing_sign', 'Large_vehicle', 'Bus',
                 'Box_truck', 'Truck', 'Vehicular_trailer', 'Truck_cab', 'School_bus', 'Articulated_bus', 'Message_board_trailer',
                 'Bicycle', 'Motorcycle', 'Wheeled_device', 'Wheelchair', 'Stroller', 'Dog']
ARGO2_GROUPS = [ARGO2_CLASSES[:1], ARGO2_CLASSES[1:5], ARGO2_CLASSES[5:11], ARGO2_CLASSES[11:20], ARGO2_CLASSES[20:25],
                ARGO2_CLASSES[25:]]
ARGO2_THRESH = [0.4, 0.25, 0.25, 0.25, 0.25, 0.25]
SMALL_CLASSES = ['a', 'b', 'c']                       # 4 logits in 2 groups, the classes of a group not adjacent
SMALL_GROUPS = [['b'], ['c', 'a']]
SMALL_THRESH = [0.3, 0.45]
LAYOUTS = {'argo2': (ARGO2_CLASSES, ARGO2_GROUPS, ARGO2_THRESH), 'small': (SMALL_CLASSES, SMALL_GROUPS, SMALL_THRESH)}

thresholds32 = S.thresholds32
margin_ok = V.margin_ok
topk_extra_mask = V.topk_extra_mask
update_by_mask = S.update_by_mask
combine = S.combine
centers_f64 = V.centers_f64


def layout(name, threshold_buffer=0.0):
    """-> (class names, group names, groups as class indices, float32-rounded thresholds)"""
    classes, group_names, thresh = LAYOUTS[name]
    return classes, group_names, V.groups_by_names(group_names, classes), S.thresholds32(thresh, threshold_buffer)


def gather_group_by_names(scores, group_names, class_names):
    """:907-919"""
    return torch.stack([scores[:, [class_names.index(n) for n in g]].sum(1) for g in group_names], dim=1)


def get_offset_weight(seg_logit):
    """:883-891, mode 'max'"""
    return V.offset_weight(seg_logit)


def group_sample(data, groups, thr32, extra_mask=None):
    """:818-881 over data = dict(seg_points, seg_logits, seg_vote_preds, seg_feats, batch_idx, vote_offsets): per-group lists of
    every entry + fg_mask_list + center_preds (+ rule: did the at-least-one-point rule fire for the group)"""
    return V.group_sample(data, groups, thr32, 1, extra_mask, batched=True)


def make_case(n, name, b, seed, f=8, fg=0.3, threshold_buffer=0.0, device='cpu'):
    """a synthetic batch of the layout: every grouped float64 score clear of its float32 threshold (redrawn until it is)"""
    classes, _, groups, thr = layout(name, threshold_buffer)
    data = V.make_case(n, len(classes) + 1, b, f, seed, groups, thr, p_cols=4, fg=fg, device=device)
    assert bool(V.margin_ok(data['seg_logits'], groups, thr).all())
    return data


def with_equal_maxima(data, groups, thr, rows):
    """the two first classes of every group of two or more get the same, dominating logit in ``rows`` (two equal maxima: the
    weights are 0.5 each); the rows stay clear of the thresholds (asserted)"""
    logits = data['seg_logits'].clone()
    for gi, grp in enumerate(groups):
        if len(grp) >= 2:
            logits[rows, grp[0]] = logits[rows, grp[1]] = 2.0 + gi         # a different height per group: no score near 1 / G
    assert bool(V.margin_ok(logits, groups, thr).all()), 'an equal-maxima row is ambiguous against its threshold'
    return dict(data, seg_logits=logits)
