"""Times the deformable convolution (csrc/deform_conv.hip) at the shipped shape of CenterHead's DCNSeparateHead - batch 2,
64 -> 64 channels, groups 4, 3 x 3, padding 1, 468 x 468 - with device events after warm-up (the median of --iters separately
timed calls, the middle one of three alternating rounds), next to the same operator composed from torch ops on the same device,
which is mmcv's algorithm: a bilinear gather into the [B, Cin * 9, H * W] column buffer, a grouped matmul, and autograd for the
backward (index_add of the gathers, the matmuls transposed).  Also the whole CenterHead (attach_network(): shared convolution,
two deformable convolutions, six head branches) forward + loss + backward at that size.  Prints one JSON object.

    python tools/deform_conv_bench.py [--iters 10] [--out profiles/deform_conv/deform_conv_bench.json]

Per fused call: milliseconds (a call time by device events, launch gaps inside), the bytes the call has to move computed from the
shapes and those bytes over the time as a fraction of the 8 TB/s HBM roof of the MI355X; peak device memory above the operands of
one forward + backward of either path.
"""
import argparse
import ast
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bench_common import median_ms  # noqa: E402
import sst_amd  # noqa: E402

DEV = 'cuda:0'
HBM_BYTES_PER_S = 8.0e12
B, C, H, W, GROUPS, K, PAD = 2, 64, 468, 468, 4, 3, 1


def composed_deform_conv(x, offset, weight):
    """mmcv's data flow in torch ops (deform_groups 1, stride 1, dilation 1): columns [B, Cin * 9, H * W], grouped matmul"""
    kk, hw = K * K, H * W
    dev = x.device
    off = offset.view(B, 1, kk, 2, hw)
    taps = torch.arange(kk, device=dev)
    pix = torch.arange(hw, device=dev)
    base_h = ((pix // W) - PAD)[None, :] + (taps // K)[:, None]
    base_w = ((pix % W) - PAD)[None, :] + (taps % K)[:, None]
    h, w = base_h + off[:, :, :, 0], base_w + off[:, :, :, 1]
    valid = (h > -1) & (w > -1) & (h < H) & (w < W)
    hl, wl = torch.floor(h), torch.floor(w)
    lh, lw = h - hl, w - wl
    flat = x.view(B, C, hw)
    col = None
    for dy, dx, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
        y, xx = hl + dy, wl + dx
        inside = valid & (y >= 0) & (y <= H - 1) & (xx >= 0) & (xx <= W - 1)
        idx = (y.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long()
        v = flat.gather(2, idx.expand(B, C, kk, hw).reshape(B, C, kk * hw)).view(B, C, kk, hw)
        term = v * (wt * inside)
        col = term if col is None else col + term
    col = col.view(B, GROUPS, C // GROUPS * kk, hw)
    out = torch.matmul(weight.view(GROUPS, C // GROUPS, C // GROUPS * kk), col)
    return out.view(B, C, H, W)


def peak_extra(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def center_head_step():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'configs', 'sst_refactor',
                        'sst_waymoD5_1x_3class_centerhead.model.py')
    model = ast.literal_eval(open(path).read())
    torch.manual_seed(0)
    head = sst_amd.build_head(dict(model['bbox_head'], train_cfg=model['train_cfg'], test_cfg=model['test_cfg']))
    head = head.attach_network().to(DEV).train()
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, sst_amd.DeformConv2dPack):
                m.conv_offset.weight.normal_(0, 0.02)
    g = torch.Generator().manual_seed(2)
    feats = torch.randn(B, 128, H, W, generator=g).to(DEV).requires_grad_()
    boxes, labels = [], []
    for _ in range(B):
        b = torch.zeros(100, 9)
        b[:, :2] = (torch.rand(100, 2, generator=g) - 0.5) * 146
        b[:, 2] = -1.5 + torch.rand(100, generator=g)
        b[:, 3:6] = torch.tensor([2.0, 4.5, 1.7]) * (0.4 + torch.rand(100, 3, generator=g))
        b[:, 6] = torch.rand(100, generator=g) * 6.28 - 3.14
        boxes.append(b.to(DEV))
        labels.append(torch.randint(0, 3, (100,), generator=g).to(DEV))

    def step():
        head.zero_grad(set_to_none=True)
        feats.grad = None
        losses = head.loss(boxes, labels, head([feats]))
        sum(losses.values()).backward()
        return losses
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, C, H, W, generator=g).to(DEV).requires_grad_()
    offset = (torch.randn(B, 2 * K * K, H, W, generator=g) * 2.0).to(DEV).requires_grad_()
    weight = (torch.randn(C, C // GROUPS, K, K, generator=g) / 12.0).to(DEV).requires_grad_()
    gout = torch.randn(B, C, H, W, generator=g).to(DEV)
    leaves = (x, offset, weight)

    def fused_fwd():
        with torch.no_grad():
            return sst_amd.deform_conv2d(x, offset, weight, padding=PAD, groups=GROUPS)

    def composed_fwd():
        with torch.no_grad():
            return composed_deform_conv(x, offset, weight)

    def fused():
        return torch.autograd.grad(sst_amd.deform_conv2d(x, offset, weight, padding=PAD, groups=GROUPS), leaves, gout)

    def composed():
        return torch.autograd.grad(composed_deform_conv(x, offset, weight), leaves, gout)

    a, b = fused_fwd(), composed_fwd()
    gap = dict(out=float((a - b).abs().max() / b.abs().max()))
    ga, gb = fused(), composed()
    for name, p, q in zip(('input_grad', 'offset_grad', 'weight_grad'), ga, gb):
        gap[name] = float((p - q).abs().max() / q.abs().max())
    del a, b, ga, gb
    step = center_head_step()
    rounds = {k: [] for k in ('fused_fwd', 'composed_fwd', 'fused', 'composed', 'center_head_step')}
    few = max(args.iters // 3, 3)
    for _ in range(3):                       # alternate the paths: other work shares the machine
        rounds['fused_fwd'].append(median_ms(fused_fwd, args.iters))
        rounds['composed_fwd'].append(median_ms(composed_fwd, few, warmup=1))
        rounds['fused'].append(median_ms(fused, args.iters))
        rounds['composed'].append(median_ms(composed, few, warmup=1))
        rounds['center_head_step'].append(median_ms(step, few, warmup=1))
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, shape=dict(batch=B, channels=C, groups=GROUPS, kernel=K,
                                                                                 map=[H, W]),
               statistic='median of device-event call times, the middle one of three alternating rounds',
               max_gap_fused_vs_composed_over_max=gap)
    for k, v in rounds.items():
        res[k + '_ms'] = round(sorted(m for m, _ in v)[1], 4)
        res[k + '_min_ms'] = round(min(m for _, m in v), 4)
    res['fused_bwd_ms'] = round(res['fused_ms'] - res['fused_fwd_ms'], 4)
    res['composed_over_fused_fwd'] = round(res['composed_fwd_ms'] / res['fused_fwd_ms'], 2)
    res['composed_over_fused'] = round(res['composed_ms'] / res['fused_ms'], 2)
    nx, noff, nout = x.numel() * 4, offset.numel() * 4, gout.numel() * 4
    # forward: operands read once, output written once.  backward: two passes over input, offsets and gout (column / offset /
    # input gradient; weight gradient), the int64 image zeroed, accumulated and read (8 B per input element each), both gradients
    nbytes = dict(fused_fwd=nx + noff + nout, fused_bwd=2 * (nx + noff + nout) + 3 * 2 * nx + nx + noff)
    res['algorithmic_bytes'] = nbytes
    res['column_buffer_bytes'] = B * C * K * K * H * W * 4
    res['fraction_of_hbm_roof'] = {k: round(v / (res[k + '_ms'] * 1e-3) / HBM_BYTES_PER_S, 4) for k, v in nbytes.items()}
    res['peak_extra_bytes'] = dict(fused_fwd=peak_extra(fused_fwd), composed_fwd=peak_extra(composed_fwd),
                                   fused=peak_extra(fused), composed=peak_extra(composed))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
