"""The fused SIR stage: Linear (no bias) -> LayerNorm -> activation -> max pooling over the points of a cluster as ONE
forward and ONE backward kernel (csrc/sir_stage.hip) instead of a library GEMM, the LayerNorm row kernel, the tile reduction
and the gather + concat of voxel_encoders/voxel_encoder.py:738-750 (layers: voxel_encoders/utils.py:147-189).

A later stage of a SIRLayer reads ``cat([point_feats, pooled[unq_inv]])`` (voxel_encoder.py:744-747); its linear splits into
``point_feats W[:, :128]^T + (pooled W[:, 128:]^T)[unq_inv]``, so that stage is ``sir_stage(point_feats, W[:, :128], ...,
add_rows=tall_linear(pooled, W[:, 128:]))`` and the [N, 256] matrix is never formed (as vfe_fused.py does for DynamicVFE).

The fused product (exact fp32 on the matrix pipe, K in ascending chunks) rounds differently from the library GEMM of the
composed path, so ``SIRLayer.fused_stage`` is OFF by default; ``enable_fused_sir(module)`` switches every SIRLayer below a module.
"""
import torch
from torch import nn
from torch.autograd import Function

from . import _lib
from . import kernels as K
from .dense import _LN_ACTS, _act_name, weight_bias_grad

SIR_STAGE_WIDTH = 128    # output width the kernel is built for (every shipped FSD / FSDv2 SIR config)
SIR_STAGE_MAX_K = 256    # widest input


def sir_stage_tile_rows():
    """sorted positions per workgroup of the forward kernel: a group that crosses a multiple of it is merged across workgroups"""
    return int(_lib.load().sst_sir_stage_tile_rows())


class _SirStage(Function):
    """(y, pooled) = stage(x, weight, gamma, beta, add_rows); saves x, weight, pre, stats, argmax"""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, add_rows, eps, act, plan):
        n, k = x.shape
        m = int(plan.m)
        dev = x.device
        pre = torch.empty((n, SIR_STAGE_WIDTH), dtype=torch.float32, device=dev)
        y = torch.empty_like(pre)
        stats = torch.empty((n, 2), dtype=torch.float32, device=dev)
        pooled = torch.empty((m, SIR_STAGE_WIDTH), dtype=torch.float32, device=dev)
        argmax = torch.empty((m, SIR_STAGE_WIDTH), dtype=torch.int32, device=dev)
        scratch = K._long_group_scratch(plan, n, m, SIR_STAGE_WIDTH, dev)
        rc = _lib.load().sst_sir_gather_segmax_fwd_f32(
            _lib.ptr(x), n, k, _lib.ptr(weight), weight.stride(0), weight.size(0), _lib.ptr(add_rows), _lib.ptr(gamma),
            _lib.ptr(beta), float(eps), _LN_ACTS[act], _lib.ptr(plan.perm), _lib.ptr(plan.inverse), _lib.ptr(plan.offsets), m,
            _lib.ptr(scratch), _lib.ptr(pre), _lib.ptr(stats), _lib.ptr(y), _lib.ptr(pooled), _lib.ptr(argmax),
            _lib.stream_ptr())
        _lib.check(rc, 'sst_sir_gather_segmax_fwd_f32')
        ctx.save_for_backward(x, weight, pre, stats, argmax, gamma, beta)
        ctx.plan, ctx.act, ctx.has_add = plan, act, add_rows is not None
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(argmax, pre, stats)   # handed out for inspection (return_saved), not part of the graph
        return y, pooled, argmax, pre, stats

    @staticmethod
    def backward(ctx, dy, dpooled, _dargmax=None, _dpre=None, _dstats=None):
        x, weight, pre, stats, argmax, gamma, beta = ctx.saved_tensors
        plan = ctx.plan
        n, m = pre.size(0), int(plan.m)
        dev = pre.device
        dy = dy.contiguous() if dy is not None else None
        dpooled = dpooled.contiguous() if dpooled is not None else None
        d_pre = torch.empty_like(pre)
        dgamma = torch.empty(SIR_STAGE_WIDTH, dtype=torch.float32, device=dev)
        dbeta = torch.empty(SIR_STAGE_WIDTH, dtype=torch.float32, device=dev)
        lib = _lib.load()
        ws = _lib.workspace(lib.sst_sir_gather_segmax_bwd_workspace_bytes(n), dev)
        rc = lib.sst_sir_gather_segmax_bwd_f32(_lib.ptr(dy), _lib.ptr(dpooled), _lib.ptr(argmax), _lib.ptr(plan.inverse),
                                               _lib.ptr(pre), _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta),
                                               _LN_ACTS[ctx.act], n, SIR_STAGE_WIDTH, m, _lib.ptr(d_pre), _lib.ptr(dgamma),
                                               _lib.ptr(dbeta), _lib.ptr(ws), _lib.stream_ptr())
        _lib.check(rc, 'sst_sir_gather_segmax_bwd_f32')
        dx = dw = dadd = None
        if ctx.needs_input_grad[0]:
            dx = d_pre @ weight
        if ctx.needs_input_grad[1]:
            dw = weight_bias_grad(d_pre, x, False)[0]
        if ctx.has_add and ctx.needs_input_grad[4]:
            dadd = K.segment_reduce(d_pre, plan, 'sum')      # every point of a group read the group's row
        return dx, dw, dgamma, dbeta, dadd, None, None, None


def _check_stage_inputs(x, weight, norm, plan, add_rows):
    _lib.require_cuda(x, norm.weight, norm.bias, add_rows)
    if not weight.is_cuda:
        raise RuntimeError('sst_amd: tensor must be a CUDA/HIP tensor (no CPU path in this library)')
    if x.dim() != 2 or weight.dim() != 2 or x.dtype != torch.float32 or weight.dtype != torch.float32:
        raise RuntimeError('sst_amd.sir_stage: x [N, K] and weight [128, K] must be 2-D float32 tensors')
    if weight.size(0) != SIR_STAGE_WIDTH or weight.size(1) != x.size(1) or not 1 <= x.size(1) <= SIR_STAGE_MAX_K \
            or weight.stride(1) != 1:
        raise RuntimeError('sst_amd.sir_stage: weight must be [128, K] with unit column stride, 1 <= K <= 256')
    if plan.m is None or plan.n != x.size(0):
        raise RuntimeError('sst_amd.sir_stage: the plan must group exactly the rows of x and know its group count')
    if add_rows is not None and (add_rows.shape != (plan.m, SIR_STAGE_WIDTH) or add_rows.dtype != torch.float32):
        raise RuntimeError('sst_amd.sir_stage: add_rows must be float32 [groups, 128]')


def sir_stage(x, weight, norm, act, plan, add_rows=None, return_saved=False):
    """-> (y [N, 128], pooled [M, 128]) of one SIR stage over the grouping ``plan`` (a kernels.UniquePlan without empty groups):

        pre = x @ weight.T (+ add_rows[plan.inverse]);  y = act(norm(pre));  pooled[g] = max of y over the rows of group g

    norm: an nn.LayerNorm(128) with affine parameters; act: None, 'relu', 'gelu' or an nn.ReLU / exact nn.GELU / nn.Identity
    module.  weight may be a column slice of a wider matrix (row stride > K).  return_saved: also return what the node saved,
    (argmax [M, 128] int32 row indices - the smallest row attaining the maximum -, pre [N, 128], stats [N, 2])."""
    if not isinstance(norm, nn.LayerNorm) or not norm.elementwise_affine or norm.bias is None \
            or tuple(norm.normalized_shape) != (SIR_STAGE_WIDTH,):
        raise RuntimeError('sst_amd.sir_stage: norm must be an affine nn.LayerNorm over the last dimension of width 128')
    name = act if (act is None or isinstance(act, str)) else _act_name(act)
    if name not in _LN_ACTS:
        raise RuntimeError('sst_amd.sir_stage: the activation must be None, ReLU or the exact (erf) GELU')
    _check_stage_inputs(x, weight, norm, plan, add_rows)
    y, pooled, argmax, pre, stats = _SirStage.apply(x.contiguous(), weight, norm.weight, norm.bias,
                                                     add_rows.contiguous() if add_rows is not None else None,
                                                     norm.eps, name, plan)
    if return_saved:
        return y, pooled, (argmax, pre, stats)
    return y, pooled


def sir_stage_ok(x, linear, norm, act, dropout, mode, plan, k_in=None):
    """can ``sir_stage`` stand in for Linear -> norm -> act -> pooling of one stage?  fp32 CUDA input; nn.LayerNorm over the last
    dimension with affine parameters; a 128-wide Linear without bias reading K <= 256 columns of x; act None / ReLU / exact GELU
    (a module, or the strings 'relu' / 'gelu'); no active dropout; max pooling; a grouping produced by this library's
    sorted-unique (no empty groups: a plan rebuilt from a foreign inverse is not eligible).
    k_in: the Linear's input width when x holds only its first columns (the split second stage); default x.size(1)."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32):
        return False
    if not isinstance(linear, nn.Linear) or linear.bias is not None or linear.out_features != SIR_STAGE_WIDTH:
        return False
    if linear.in_features != (x.size(1) if k_in is None else k_in) or not 1 <= x.size(1) <= SIR_STAGE_MAX_K \
            or linear.weight.dtype != torch.float32 or not linear.weight.is_cuda:
        return False
    if not isinstance(norm, nn.LayerNorm) or not norm.elementwise_affine or norm.bias is None \
            or tuple(norm.normalized_shape) != (SIR_STAGE_WIDTH,):
        return False
    name = act if (act is None or isinstance(act, str)) else _act_name(act)
    if name is False or name not in _LN_ACTS:
        return False
    if dropout is not None and dropout.training and dropout.p > 0:
        return False
    if mode != 'max':
        return False
    return (plan is not None and getattr(plan, 'native', False) and plan.m is not None and plan.m > 0
            and plan.n == x.size(0) and x.size(0) > 0)


def enable_fused_sir(module, flag=True):
    """set ``fused_stage`` on every SIRLayer below ``module`` (the module itself included); returns the module"""
    from .voxel_encoder import SIRLayer
    for sub in module.modules():
        if isinstance(sub, SIRLayer):
            sub.fused_stage = bool(flag)
    return module
