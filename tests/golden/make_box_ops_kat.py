"""Writes tests/golden/box_ops_kat.npz: the literal inputs and expected outputs of the reference's own known-answer tests
of its rotated-box kernels (numbers only), read out of the reference's test sources with `ast`:

- tests/test_utils/test_box3d.py::test_boxes3d_overlaps               -> iou_boxes1 / iou_boxes2 / iou_expected / iof_expected
- tests/test_models/test_common_modules/test_roiaware_pool3d.py::
    test_points_in_boxes_gpu                                         -> pib_gpu_boxes / pib_gpu_pts / pib_gpu_expected
    test_points_in_boxes_batch                                       -> pib_batch_boxes / pib_batch_pts / pib_batch_expected
- tests/test_models/test_heads/test_parta2_bbox_head.py::test_multi_class_nms
                                                                     -> mcn_probs / mcn_preds / mcn_expected

Those expected values were produced by runs of the reference's CUDA kernels.

    python tests/golden/make_box_ops_kat.py /path/to/reference
"""
import ast
import os
import sys

import numpy as np

SOURCES = {
    'test_boxes3d_overlaps': ('tests/test_utils/test_box3d.py', {
        'boxes1_tensor': 'iou_boxes1', 'boxes2_tensor': 'iou_boxes2', 'expected_iou_tensor': 'iou_expected',
        'expected_iof_tensor': 'iof_expected'}),
    'test_points_in_boxes_gpu': ('tests/test_models/test_common_modules/test_roiaware_pool3d.py', {
        'boxes': 'pib_gpu_boxes', 'pts': 'pib_gpu_pts', 'expected_point_indices': 'pib_gpu_expected'}),
    'test_points_in_boxes_batch': ('tests/test_models/test_common_modules/test_roiaware_pool3d.py', {
        'boxes': 'pib_batch_boxes', 'pts': 'pib_batch_pts', 'expected_point_indices': 'pib_batch_expected'}),
    'test_multi_class_nms': ('tests/test_models/test_heads/test_parta2_bbox_head.py', {
        'box_probs': 'mcn_probs', 'box_preds': 'mcn_preds', 'expected_selected': 'mcn_expected'}),
}
DTYPES = {'pib_gpu_expected': np.int32, 'pib_batch_expected': np.int32, 'mcn_expected': np.int64}


def _tensor_literal(node):
    """the first argument of torch.tensor(...) / torch.Tensor(...), possibly under a .cuda() / .to() chain"""
    while isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in ('cuda', 'to'):
        node = node.func.value
    if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in ('tensor', 'Tensor')
            and node.args):
        return ast.literal_eval(node.args[0])
    return None


def extract(reference_root):
    out = {}
    for fn_name, (rel, names) in SOURCES.items():
        tree = ast.parse(open(os.path.join(reference_root, rel)).read())
        fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == fn_name)
        for stmt in ast.walk(fn):
            if isinstance(stmt, ast.Assign) and len(stmt.targets) == 1 and isinstance(stmt.targets[0], ast.Name):
                key = names.get(stmt.targets[0].id)
                if key is None or key in out:
                    continue
                val = _tensor_literal(stmt.value)
                if val is not None:
                    out[key] = np.asarray(val, dtype=DTYPES.get(key, np.float32))
        missing = [k for k in names.values() if k not in out]
        if missing:
            raise RuntimeError(f'{rel}::{fn_name}: literals not found: {missing}')
    return out


if __name__ == '__main__':
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('SST_REFERENCE_ROOT', '')
    arrays = extract(ref)
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'box_ops_kat.npz')
    np.savez(dst, **arrays)
    for k, v in sorted(arrays.items()):
        print(f'{k:20s} {v.dtype} {v.shape}')
