"""What the head modules (seg_loss, center_head, cluster_head, roi_head, anchor_head) share on the host side: the input checks,
the config getter, the world size, the prefix offsets of a batch and the phases of the two-phase loss forwards."""
import torch

from . import _lib

# phases of sst_cluster_loss_fwd_f32 / sst_roi_loss_fwd_f32 (SST_CLUSTER_LOSS_* / SST_ROI_LOSS_* of include/sst_amd.h)
LOSS_COUNTS, LOSS_FINISH = 1, 2


def check_f32(where, *tensors):
    """device float32 tensors (None is skipped), or RuntimeError; ``where``: the 'sst_amd.cluster_head' prefix of the message"""
    _lib.require_cuda(*tensors)
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError(f'{where}: float32 tensors expected, got {t.dtype}')


def check(where, t, dtype, shape, what):
    _lib.require_cuda(t)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise RuntimeError(f'{where}: {what} must be {dtype} of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}')


def cfg_get(cfg, key, default=None):
    """mmcv's ConfigDict answers both cfg['a'] and cfg.a; plain dicts (what the tests exec from the config text) only the first"""
    if cfg is None:
        return default
    return cfg.get(key, default) if hasattr(cfg, 'get') else getattr(cfg, key, default)


def dist_world():
    dist = torch.distributed
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size()
    return 1


def offsets(sizes, device):
    """-> (int32 device tensor [len(sizes) + 1] of the prefix sums, total)"""
    off = [0]
    for s in sizes:
        off.append(off[-1] + int(s))
    return torch.tensor(off, dtype=torch.int32).to(device, non_blocking=True), off[-1]
