#!/usr/bin/env python
"""Per-layer times of the sparse convolutions of a bench workload in the multiply modes of the output-stationary kernels: fp32
matrix pipe (csrc/spconv_os.hip), exact three-way bf16 split (csrc/spconv_os_x6.hip, the default), two-way split
(csrc/spconv_os_x3.hip, forward only) and bf16 operands (csrc/spconv_os_bf16.hip).  For every layer shape: forward, data-gradient
and filter-gradient time, and the error of 'f32x6' and 'bf16' against the float64 contraction of the unrounded operands, relative
to the largest reference element; then the workload's whole sparse U-Net, forward + backward, at 'f32x6' and at 'bf16' - all in
one process, the modes interleaved per layer.
Usage: python tools/conv_modes.py [fsd|fsdv2] [points] [--json out.json]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_workloads as BW  # noqa: E402
from sst_amd import sparse_unet as SU  # noqa: E402
from sst_amd import spconv as SP  # noqa: E402
from tools.conv_layers import timeit  # noqa: E402

DEV = torch.device('cuda:0')
MODES = ('f32', 'f32x6', 'f32x3', 'bf16')


def conv64(x, mp, w3):
    """float64: Y[r] = sum_k X[mp[k][r]] W[k]"""
    xd, wd = x.double(), w3.double()
    y = torch.zeros(mp.size(1), w3.size(2), dtype=torch.float64, device=x.device)
    for k in range(mp.size(0)):
        rows = torch.nonzero(mp[k] >= 0)[:, 0]
        if rows.numel():
            y.index_add_(0, rows, xd[mp[k][rows].long()] @ wd[k])
    return y


def wgrad64(x, dy, pairs, num, x_side):
    dw = torch.zeros(len(num), x.size(1), dy.size(1), dtype=torch.float64, device=x.device)
    for k, n in enumerate(num):
        if n:
            dw[k] = x.double()[pairs[k, x_side, :n].long()].t() @ dy.double()[pairs[k, 1 - x_side, :n].long()]
    return dw


def rel_err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    out_json = sys.argv[sys.argv.index('--json') + 1] if '--json' in sys.argv else None
    if out_json in args:
        args.remove(out_json)
    what = args[0] if args else 'fsd'
    spec = BW.WORKLOADS[what]
    n_pts = int(args[1]) if len(args) > 1 else spec['points']
    torch.manual_seed(0)
    model = spec['cls']().to(DEV).train()
    clouds = [model.make_cloud(n_pts, 0, DEV)]
    layers, names, unet_call = [], {}, {}

    def post(mod, inp, out):
        datas = out.indice_dict.get(mod.indice_key) if (mod.indice_key is not None and not mod.conv1x1) else None
        rb = getattr(datas[2], '_sst_rulebook', None) if datas is not None else None
        if rb is not None:
            layers.append((mod, inp[0].features.detach(), rb, datas[2]))

    def unet_pre(mod, a, kw):
        unet_call.setdefault('net', mod)
        unet_call.setdefault('args', (a, kw))

    for name, m in model.named_modules():
        if isinstance(m, SP.SparseConvolution):
            m.register_forward_hook(post)
            names[m] = name
        if isinstance(m, SU._UNetStages):
            m.register_forward_pre_hook(unet_pre, with_kwargs=True)
    with torch.no_grad():
        model(clouds)
    torch.cuda.synchronize()
    result = dict(workload=what, points=n_pts, modes=list(MODES), layers=[],
                  how='hip events around one call, median of 10 after 3 warm-up calls, milliseconds; errors: max |mode - float64| / '
                      'max |float64| on the unrounded operands of the layer as the workload ran it (dY: unit normal)')
    tot = {(m, p): 0.0 for m in MODES for p in ('fwd', 'dgrad', 'wgrad')}
    seen = {}
    print(f'{"layer":34s} {"rows":>7s} {"cin":>4s} {"cout":>4s} {"pairs":>8s} | fwd us: f32 x6 x3 bf16 | dgrad us: f32 x6 bf16 | '
          f'wgrad us: f32 x6 bf16 | rel err fwd/dgrad/wgrad: x6 | bf16')
    for mod, x, rb, pairs in layers:
        cin, cout = mod.in_channels, mod.out_channels
        w3 = mod.weight.detach().reshape(-1, cin, cout)
        (fmap, frows, bmap, brows, x_side) = ((rb.in2out, rb.n, rb.out2in, rb.m, 1) if mod.inverse
                                              else (rb.out2in, rb.m, rb.in2out, rb.n, 0))
        gy = torch.randn(frows, cout, device=DEV)
        t = {}
        for mode in MODES:
            t[mode, 'fwd'] = timeit(lambda: SP._gather_gemm(x, fmap, frows, w3, False, cout, rb, precision=mode))
            if mode != 'f32x3':        # the two-way split is a forward leg only
                t[mode, 'dgrad'] = timeit(lambda: SP._gather_gemm(gy, bmap, brows, w3, True, cin, rb, precision=mode))
                t[mode, 'wgrad'] = timeit(lambda: SP._wgrad(x, gy, rb, pairs, x_side, tuple(w3.shape), precision=mode))
            for p in ('fwd', 'dgrad', 'wgrad'):
                tot[mode, p] += t.get((mode, p), 0.0)
        key = (frows, cin, cout, rb.total_pairs, bool(mod.inverse))
        err = seen.get(key)
        if err is None:               # one float64 reference per layer SHAPE (layers of a level share rulebook and widths)
            num = [int(v) for v in rb.num.cpu()]
            refs = (conv64(x, fmap, w3), conv64(gy, bmap, w3.transpose(1, 2)), wgrad64(x, gy, pairs, num, x_side))
            err = {}
            for mode in ('f32x6', 'bf16'):
                got = (SP._gather_gemm(x, fmap, frows, w3, False, cout, rb, precision=mode),
                       SP._gather_gemm(gy, bmap, brows, w3, True, cin, rb, precision=mode),
                       SP._wgrad(x, gy, rb, pairs, x_side, tuple(w3.shape), precision=mode))
                err[mode] = [rel_err(g, r) for g, r in zip(got, refs)]
            seen[key] = err
            del refs
        us = lambda m, p: t[m, p] * 1e3     # noqa: E731
        print(f'{names[mod][-34:]:34s} {frows:7d} {cin:4d} {cout:4d} {rb.total_pairs:8d} | '
              f'{us("f32", "fwd"):6.0f} {us("f32x6", "fwd"):6.0f} {us("f32x3", "fwd"):6.0f} {us("bf16", "fwd"):6.0f} | '
              f'{us("f32", "dgrad"):6.0f} {us("f32x6", "dgrad"):6.0f} {us("bf16", "dgrad"):6.0f} | '
              f'{us("f32", "wgrad"):6.0f} {us("f32x6", "wgrad"):6.0f} {us("bf16", "wgrad"):6.0f} | '
              + ' '.join('%.1e' % e for e in err['f32x6']) + ' | ' + ' '.join('%.1e' % e for e in err['bf16']))
        result['layers'].append(dict(name=names[mod], rows=frows, cin=cin, cout=cout, pairs=rb.total_pairs, inverse=bool(mod.inverse),
                                     ms={f'{m}_{p}': round(v, 5) for (m, p), v in t.items()},
                                     rel_err={m: dict(zip(('fwd', 'dgrad', 'wgrad'), e)) for m, e in err.items()}))
    result['total_ms'] = {f'{m}_{p}': round(v, 4) for (m, p), v in tot.items()}
    for p in ('fwd', 'dgrad', 'wgrad'):
        print(f'total {p} ms: ' + ', '.join(f'{m} {tot[m, p]:.2f}' for m in MODES if tot[m, p] > 0))
    # the whole U-Net, forward + backward, rulebooks rebuilt per call as in a training step
    if unet_call:
        net = unet_call['net']
        a, kw = unet_call['args']

        def step():
            net.zero_grad(set_to_none=True)
            out = net(*a, **kw)
            feats = out[0]['voxel_feats'] if isinstance(out, list) else (out['seg_features'] if isinstance(out, dict) else out[0])
            feats.square().mean().backward()

        unet = {}
        for rnd in range(2):          # two interleaved rounds: drift of the box shows as a gap between them
            for mode in ('f32x6', 'bf16'):
                net.set_precision(mode)
                unet.setdefault(mode, []).append(round(timeit(step), 4))
        net.set_precision(None)
        result['unet_fwd_bwd_ms'] = unet
        print('U-Net forward + backward ms (two rounds): ' + ', '.join(f'{m} {v}' for m, v in unet.items()))
    if out_json:
        os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
        with open(out_json, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
