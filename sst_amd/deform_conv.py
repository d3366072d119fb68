"""Deformable convolution v1 (csrc/deform_conv.hip): ``deform_conv2d``, ``DeformConv2d`` and ``DeformConv2dPack``.

Reference: mmcv.ops.deform_conv (deform_conv2d, DeformConv2d, DeformConv2dPack = the ``'DCN'`` of mmcv's CONV_LAYERS), used by
DCNSeparateHead of mmdet3d/models/dense_heads/centerpoint_head.py:123-239 through ``build_conv_layer(dcn_config)``.  The
conventions (written out in include/sst_amd.h and restated in float64 by tests/deform_conv_ref.py):

    h = ho * stride_h - pad_h + i * dil_h + off_h,  w = wo * stride_w - pad_w + j * dil_w + off_w
    off_h / off_w = channels 2 (i kw + j) / 2 (i kw + j) + 1 of the block of deformable group c // (Cin // deform_groups)
    sample = 0 unless h > -1 and w > -1 and h < H and w < W, else bilinear over the cell (floor(h), floor(w)), outside corners 0
    weight [Cout, Cin / groups, kh, kw]; no bias, no modulation mask

One launch forward without a column buffer; the backward writes all three gradients without float atomics (two runs agree bit
for bit).  fp32 device tensors only, kernels up to 3 x 3; CPU tensors, other dtypes, ``bias=True`` and the modulated 'DCNv2' are
refused by name.  Nothing compiled from mmcv was available to compare with: parity is pinned to the definition above and to
two identities (zero offsets = F.conv2d, integer offsets = a convolution of shifted zero-padded input), DESIGN.md 3.20.
"""
import ctypes
import math

import torch
from torch import nn
from torch.nn.modules.utils import _pair

from . import _lib


def deform_conv_tile_pixels():
    """output pixels per workgroup (consecutive pixels of one sample)"""
    return int(_lib.load().sst_deform_conv_tile_pixels())


def deform_conv_wgrad_blocks(total_tiles):
    """blocks along the tiles of the weight gradient's grid: block x takes the tiles x, x + blocks, ... (current device)"""
    return int(_lib.load().sst_deform_conv_wgrad_blocks(int(total_tiles)))


def _shape_of(input, weight, stride, padding, dilation, groups, deform_groups):
    b, cin, h, w = input.shape
    cout, _, kh, kw = weight.shape
    return _lib.DeformConvShape(b, cin, h, w, cout, kh, kw, stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1],
                                groups, deform_groups, 0)


class _DeformConv2d(torch.autograd.Function):

    @staticmethod
    def forward(ctx, input, offset, weight, shape, out_hw):
        out = torch.empty((input.size(0), weight.size(0), *out_hw), dtype=torch.float32, device=input.device)
        _lib.check(_lib.load().sst_deform_conv_fwd_f32(ctypes.byref(shape), _lib.ptr(input), _lib.ptr(offset), _lib.ptr(weight),
                                                       _lib.ptr(out), _lib.stream_ptr()), 'sst_deform_conv_fwd_f32')
        ctx.save_for_backward(input, offset, weight)
        ctx.shape = shape
        return out

    @staticmethod
    def backward(ctx, gout):
        input, offset, weight = ctx.saved_tensors
        gout = gout.to(torch.float32).contiguous()
        lib = _lib.load()
        nbytes = lib.sst_deform_conv_bwd_workspace_bytes(ctypes.byref(ctx.shape))
        if nbytes < 0:
            _lib.check(int(nbytes), 'sst_deform_conv_bwd_workspace_bytes')
        gin, goff, gw = torch.empty_like(input), torch.empty_like(offset), torch.empty_like(weight)
        ws = _lib.workspace(nbytes, input.device)
        _lib.check(lib.sst_deform_conv_bwd_f32(ctypes.byref(ctx.shape), _lib.ptr(input), _lib.ptr(offset), _lib.ptr(weight),
                                               _lib.ptr(gout), _lib.ptr(gin), _lib.ptr(goff), _lib.ptr(gw), _lib.ptr(ws),
                                               _lib.stream_ptr()), 'sst_deform_conv_bwd_f32')
        return gin, goff, gw, None, None


def deform_conv2d(input, offset, weight, stride=1, padding=0, dilation=1, groups=1, deform_groups=1):
    """mmcv.ops.deform_conv2d: input [B, Cin, H, W], offset [B, deform_groups * 2 * kh * kw, Ho, Wo], weight
    [Cout, Cin / groups, kh, kw] -> [B, Cout, Ho, Wo]; gradients to all three.  fp32 device tensors; kh, kw <= 3."""
    for name, t in (('input', input), ('offset', offset), ('weight', weight)):
        if not torch.is_tensor(t) or t.dim() != 4:
            raise RuntimeError(f'deform_conv2d: {name} must be a 4-D tensor')
        if t.dtype != torch.float32:
            raise RuntimeError(f'deform_conv2d: fp32 tensors only, {name} is {t.dtype} (no reduced-precision deformable '
                               'convolution is built)')
        if not t.is_cuda:
            raise RuntimeError('sst_amd: tensor must be a CUDA/HIP tensor (no CPU path in this library)')
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    groups, deform_groups = int(groups), int(deform_groups)
    cout, cg, kh, kw = weight.shape
    if kh > 3 or kw > 3:
        raise NotImplementedError(f'deform_conv2d: kernel {kh} x {kw}: kernels above 3 x 3 are not built')
    cin = input.size(1)
    if groups < 1 or deform_groups < 1 or cin % groups or cout % groups or cin % deform_groups or cg != cin // groups:
        raise RuntimeError(f'deform_conv2d: groups {groups} / deform_groups {deform_groups} must divide the channels '
                           f'({cin} -> {cout}) and weight must be [Cout, Cin / groups, kh, kw], got {tuple(weight.shape)}')
    input, offset, weight = input.contiguous(), offset.contiguous(), weight.contiguous()
    shape = _shape_of(input, weight, stride, padding, dilation, groups, deform_groups)
    oh, ow = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(_lib.load().sst_deform_conv_out_size(ctypes.byref(shape), ctypes.byref(oh), ctypes.byref(ow)),
               'sst_deform_conv_out_size')
    want = (input.size(0), deform_groups * 2 * kh * kw, oh.value, ow.value)
    if tuple(offset.shape) != want:
        raise RuntimeError(f'deform_conv2d: offset must be [B, deform_groups * 2 * kh * kw, Ho, Wo] = {want}, got '
                           f'{tuple(offset.shape)}')
    return _DeformConv2d.apply(input, offset, weight, shape, (oh.value, ow.value))


class DeformConv2d(nn.Module):
    """mmcv.ops.DeformConv2d: the parameter ``weight`` [Cout, Cin / groups, kh, kw]; ``forward(x, offset)``"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deform_groups=1,
                 bias=False):
        super().__init__()
        if bias:
            raise NotImplementedError(f'{type(self).__name__}: bias=True is not built (mmcv\'s DeformConv2d has no bias either)')
        if in_channels % groups or out_channels % groups or in_channels % deform_groups:
            raise ValueError(f'in_channels {in_channels} / out_channels {out_channels} must be divisible by groups {groups} and '
                             f'deform_groups {deform_groups}')
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.dilation = (_pair(kernel_size), _pair(stride), _pair(padding),
                                                                      _pair(dilation))
        if max(self.kernel_size) > 3:
            raise NotImplementedError(f'{type(self).__name__}: kernel {self.kernel_size}: kernels above 3 x 3 are not built')
        self.groups, self.deform_groups = groups, deform_groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, *self.kernel_size))
        self.reset_parameters()

    def reset_parameters(self):
        # torch's Kaiming default for convolutions (nn.Conv2d.reset_parameters); mmcv's own initialiser is not reproduced
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))

    def forward(self, x, offset):
        return deform_conv2d(x, offset, self.weight, self.stride, self.padding, self.dilation, self.groups, self.deform_groups)

    def extra_repr(self):
        return (f'{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, '
                f'padding={self.padding}, dilation={self.dilation}, groups={self.groups}, deform_groups={self.deform_groups}')


class DeformConv2dPack(DeformConv2d):
    """mmcv.ops.DeformConv2dPack ('DCN'): the offsets come from ``conv_offset``, a zero-initialised convolution on the input.
    state_dict keys: ``weight``, ``conv_offset.weight``, ``conv_offset.bias``."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.conv_offset = nn.Conv2d(self.in_channels, self.deform_groups * 2 * self.kernel_size[0] * self.kernel_size[1],
                                     kernel_size=self.kernel_size, stride=self.stride, padding=self.padding,
                                     dilation=self.dilation, bias=True)
        self.init_offset()

    def init_offset(self):
        self.conv_offset.weight.data.zero_()
        self.conv_offset.bias.data.zero_()

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError('sst_amd: tensor must be a CUDA/HIP tensor (no CPU path in this library)')
        return deform_conv2d(x, self.conv_offset(x), self.weight, self.stride, self.padding, self.dilation, self.groups,
                             self.deform_groups)


def _refuse_dcnv2(*args, **kwargs):
    raise NotImplementedError("build_conv_layer: 'DCNv2' (the modulated deformable convolution) is not built; 'DCN' is")
