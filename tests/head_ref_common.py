"""What the restatements of the heads (seg_loss_ref, center_head_ref, cluster_head_ref, anchor_head_ref) share."""
import numpy as np

F = np.float32


def ulp_distance(a, b):
    """element-wise distance in float32 units in the last place (monotone integer mapping of the bit patterns)"""
    def key(v):
        i = np.ascontiguousarray(v, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))
