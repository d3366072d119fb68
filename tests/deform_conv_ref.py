"""Deformable convolution v1 restated in float64 torch: an explicit gather, the forward and the analytic gradients, on any
device.  This is the definition sst_amd.deform_conv2d is tested against (mmcv's deform_conv2d, restated from its published
kernel; nothing compiled from mmcv is available to compare with):

    for output pixel (ho, wo) and tap (i, j), k = i * kw + j:
        h = ho * stride_h - pad_h + i * dil_h + off_h        w = wo * stride_w - pad_w + j * dil_w + off_w
        off_h = offset[b, d * 2 * kh * kw + 2 * k, ho, wo]   off_w = offset[b, d * 2 * kh * kw + 2 * k + 1, ho, wo]
        d = c // (Cin // deform_groups) for input channel c
    the sample of x[b, c] at (h, w) is 0 unless h > -1 and w > -1 and h < H and w < W; otherwise the bilinear value over the cell
    (floor(h), floor(w)), corners outside the image contributing 0
    out[b, o] = sum over the channels c of o's convolution group and the taps of weight[o, c_local, i, j] * sample
    (column order c * kh * kw + i * kw + j; no bias, no modulation mask)
    the derivative in an offset is that of the cell floor() selects, and 0 where the sample is 0

``forward`` also returns A = |W| . bilinear(|x|), the absolute-value product the error bars of the fp32 kernels are stated in;
``backward`` returns the three gradients and their own absolute-value products.
"""
import torch
from torch.nn.modules.utils import _pair


def out_size(h, w, kernel, stride, padding, dilation):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = _pair(kernel), _pair(stride), _pair(padding), _pair(dilation)
    return (h + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (w + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1


class Gather(object):
    """the sampling of one call: cells, fractions, validity, and the four corners (index, weight, inside mask) per
    [B, deform_groups, taps, Ho * Wo]"""

    def __init__(self, x_shape, offset, kernel, stride, padding, dilation, deform_groups):
        b, cin, H, W = x_shape
        (kh, kw), (sh, sw), (ph, pw), (dh, dw) = _pair(kernel), _pair(stride), _pair(padding), _pair(dilation)
        kk, dg = kh * kw, deform_groups
        ho_n, wo_n = offset.shape[2:]
        assert tuple(offset.shape) == (b, dg * 2 * kk, ho_n, wo_n) and (ho_n, wo_n) == out_size(H, W, kernel, stride, padding,
                                                                                               dilation)
        dev = offset.device
        off = offset.double().reshape(b, dg, kk, 2, ho_n, wo_n)
        taps = torch.arange(kk, device=dev)
        base_h = (torch.arange(ho_n, device=dev) * sh - ph)[None, :, None] + ((taps // kw) * dh)[:, None, None]   # [kk, Ho, 1]
        base_w = (torch.arange(wo_n, device=dev) * sw - pw)[None, None, :] + ((taps % kw) * dw)[:, None, None]    # [kk, 1, Wo]
        h = (base_h.double() + off[:, :, :, 0]).reshape(b, dg, kk, -1)
        w = (base_w.double() + off[:, :, :, 1]).reshape(b, dg, kk, -1)
        self.valid = (h > -1) & (w > -1) & (h < H) & (w < W)
        hl, wl = torch.floor(h), torch.floor(w)
        self.lh, self.lw = h - hl, w - wl
        self.hh, self.hw = 1 - self.lh, 1 - self.lw
        hl = torch.where(self.valid, hl, torch.zeros_like(hl)).long()
        wl = torch.where(self.valid, wl, torch.zeros_like(wl)).long()
        self.corners = []
        for dy, dx, wt in ((0, 0, self.hh * self.hw), (0, 1, self.hh * self.lw), (1, 0, self.lh * self.hw),
                           (1, 1, self.lh * self.lw)):
            y, x = hl + dy, wl + dx
            inside = self.valid & (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
            self.corners.append((y.clamp(0, H - 1) * W + x.clamp(0, W - 1), wt, inside))
        self.dims = (b, cin, H, W, kk, dg, ho_n, wo_n)

    def per_channel(self, t):
        """[B, dg, kk, P] -> [B, Cin, kk, P]"""
        return t.repeat_interleave(self.dims[1] // self.dims[5], dim=1)

    def corner_values(self, x):
        """x [B, Cin, H, W] float64 -> the four corner values [B, Cin, kk, P], 0 outside the image / where the sample is 0"""
        b, cin, H, W, kk, dg, ho_n, wo_n = self.dims
        flat = x.reshape(b, cin, H * W)
        vals = []
        for idx, _, inside in self.corners:
            v = flat.gather(2, self.per_channel(idx).reshape(b, cin, -1)).reshape(b, cin, kk, -1)
            vals.append(v * self.per_channel(inside).to(v.dtype))
        return vals

    def columns(self, x):
        vals = self.corner_values(x)
        return sum(self.per_channel(wt) * v for (_, wt, _), v in zip(self.corners, vals))


def _grouped(weight, groups):
    cout, cg, kh, kw = weight.shape
    return weight.double().reshape(groups, cout // groups, cg * kh * kw)


def forward(x, offset, weight, stride=1, padding=0, dilation=1, groups=1, deform_groups=1):
    """-> (out [B, Cout, Ho, Wo] float64, A of the same shape, the Gather)"""
    b, cin = x.shape[:2]
    cout, cg, kh, kw = weight.shape
    g = Gather(x.shape, offset, (kh, kw), stride, padding, dilation, deform_groups)
    ho_n, wo_n = g.dims[6:]
    wg = _grouped(weight, groups)
    col = g.columns(x.double()).reshape(b, groups, cg * kh * kw, -1)
    out = torch.einsum('gor,bgrp->bgop', wg, col).reshape(b, cout, ho_n, wo_n)
    col_abs = g.columns(x.double().abs()).reshape(b, groups, cg * kh * kw, -1)
    a = torch.einsum('gor,bgrp->bgop', wg.abs(), col_abs).reshape(b, cout, ho_n, wo_n)
    return out, a, g


def backward(x, offset, weight, gout, stride=1, padding=0, dilation=1, groups=1, deform_groups=1, gather=None):
    """-> dict(gin, goff, gw: the gradients in float64; a_in, a_off, a_w: their absolute-value products)"""
    b, cin, H, W = x.shape
    cout, cg, kh, kw = weight.shape
    kk = kh * kw
    g = gather or Gather(x.shape, offset, (kh, kw), stride, padding, dilation, deform_groups)
    dg = deform_groups
    wg = _grouped(weight, groups)
    go = gout.double().reshape(b, groups, cout // groups, -1)
    x64 = x.double()
    res = {}
    for tag, wv, gv, xv in (('', wg, go, x64), ('a', wg.abs(), go.abs(), x64.abs())):
        gcol = torch.einsum('gor,bgop->bgrp', wv, gv).reshape(b, cin, kk, -1)
        col = g.columns(xv).reshape(b, groups, cg * kk, -1)
        gw = torch.einsum('bgop,bgrp->gor', gv, col).reshape(cout, cg, kh, kw)
        gin = torch.zeros(b, cin, H * W, dtype=torch.float64, device=x.device)
        for idx, wt, inside in g.corners:
            contrib = gcol * g.per_channel(wt * inside.to(wt.dtype))
            gin.scatter_add_(2, g.per_channel(idx).reshape(b, cin, -1), contrib.reshape(b, cin, -1))
        v1, v2, v3, v4 = g.corner_values(xv)
        hw, lw, hh, lh = (g.per_channel(t) for t in (g.hw, g.lw, g.hh, g.lh))
        if tag == '':
            dh_, dw_ = hw * (v3 - v1) + lw * (v4 - v2), hh * (v2 - v1) + lh * (v4 - v3)
        else:
            dh_, dw_ = hw * (v3 + v1) + lw * (v4 + v2), hh * (v2 + v1) + lh * (v4 + v3)
        valid = g.per_channel(g.valid).to(torch.float64)
        goh = (gcol * dh_ * valid).reshape(b, dg, cin // dg, kk, -1).sum(2)
        gow = (gcol * dw_ * valid).reshape(b, dg, cin // dg, kk, -1).sum(2)
        goff = torch.stack((goh, gow), 3).reshape(b, dg * 2 * kk, *offset.shape[2:])
        if tag == '':
            res.update(gin=gin.reshape(b, cin, H, W), goff=goff, gw=gw)
        else:
            res.update(a_in=gin.reshape(b, cin, H, W), a_off=goff, a_w=gw)
    return res


class RefDeformConv(torch.autograd.Function):
    """the restatement as an autograd function (float64), for torch.autograd.gradcheck of its analytic gradients"""

    @staticmethod
    def forward(ctx, x, offset, weight, cfg):
        out, _, _ = forward(x, offset, weight, **cfg)
        ctx.save_for_backward(x, offset, weight)
        ctx.cfg = cfg
        return out

    @staticmethod
    def backward(ctx, gout):
        x, offset, weight = ctx.saved_tensors
        r = backward(x, offset, weight, gout, **ctx.cfg)
        return r['gin'], r['goff'], r['gw'], None


def shifted_conv(x, weight, shifts, stride=1, padding=0, dilation=1, groups=1):
    """the identity at integer offsets that are constant over the pixels: tap k reads the zero-padded input shifted by
    shifts[k] = (a, b), i.e. x(h + a, w + b) with zeros outside the image, through an unpadded convolution whose kernel is zero
    except at tap k (the padding is part of the shifted input: a shift can bring image rows into the padding's place)"""
    import torch.nn.functional as F
    cout, cg, kh, kw = weight.shape
    H, W = x.shape[2:]
    ph, pw = _pair(padding)
    out = None
    for k, (a, b) in enumerate(shifts):
        m = max(abs(a), abs(b)) + max(ph, pw)
        big = F.pad(x, (m, m, m, m))
        xs = big[:, :, m - ph + a:m + a + H + ph, m - pw + b:m + b + W + pw]
        wk = torch.zeros_like(weight)
        wk[:, :, k // kw, k % kw] = weight[:, :, k // kw, k % kw]
        y = F.conv2d(xs, wk, None, stride, 0, dilation, groups)
        out = y if out is None else out + y
    return out
