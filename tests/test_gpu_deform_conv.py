"""sst_amd.deform_conv2d on the GPU against the float64 restatement of tests/deform_conv_ref.py (run on the device too).

Exact operands (small integers, offsets on the half-integer lattice with every border position planted): every product and sum
is exact in fp32 in any order, so the output and the three gradients must equal the restatement exactly.  General operands: the
derived bound |got - ref| <= (K + 16) * 2^-24 * A elementwise, A the absolute-value product of the same sum, K the length of the
dot product behind the element (the 16 covers the roundings of the bilinear weights and the four-corner sum):
    out   K = Cin / groups * kh * kw          input gradient   K = Cout / groups (the fixed-point sum itself is exact)
    offset gradient  K = Cin / deform_groups + Cout / groups   weight gradient  K = B * Ho * Wo
torch.autograd.gradcheck does not apply (fp32 only); the restatement's own gradients pass it in tests/test_deform_conv_host.py."""
import functools

import pytest
import torch
import torch.nn.functional as F

import deform_conv_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 2.0 ** -24


def _side_e():
    """the side of shape (e): one tile more than the weight gradient's grid has blocks along the tiles, so that block 0 takes a
    second tile"""
    import sst_amd
    tile = sst_amd.deform_conv_tile_pixels()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    side = 1
    while -(-side * side // tile) <= cus or (side * side) % tile == 0:
        side += 1
    return side


# name -> (B, Cin, Cout, H, W, kernel, stride, padding, dilation, groups, deform_groups)
def _shapes():
    s = _side_e()
    return {
        'a': (2, 8, 8, 5, 7, (3, 3), 1, 1, 1, 1, 1),
        'b': (2, 64, 64, 19, 23, (3, 3), 1, 1, 1, 4, 1),
        'c': (1, 12, 20, 9, 10, (3, 3), 2, 2, 2, 2, 2),
        'd1': (8, 8, 8, 1, 1, (1, 1), 1, 0, 1, 1, 1),
        'd70': (2, 8, 8, 1, 70, (1, 1), 1, 0, 1, 2, 2),
        'e': (1, 64, 64, s, s, (3, 3), 1, 1, 1, 4, 1),
    }


SHAPES = ('a', 'b', 'c', 'd1', 'd70', 'e')


def _cfg(shape):
    b, cin, cout, h, w, kernel, stride, padding, dilation, groups, dg = shape
    return dict(stride=stride, padding=padding, dilation=dilation, groups=groups, deform_groups=dg)


def _base_positions(shape):
    """the integer part of the sampling positions: base_h, base_w [kk, Ho, Wo]"""
    b, cin, cout, h, w, (kh, kw), stride, padding, dilation, groups, dg = shape
    ho, wo = R.out_size(h, w, (kh, kw), stride, padding, dilation)
    taps = torch.arange(kh * kw)
    base_h = (torch.arange(ho) * stride - padding)[None, :, None] + ((taps // kw) * dilation)[:, None, None]
    base_w = (torch.arange(wo) * stride - padding)[None, None, :] + ((taps % kw) * dilation)[:, None, None]
    return base_h.expand(-1, ho, wo), base_w.expand(-1, ho, wo), ho, wo


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """-> (x, offset, weight, gout fp32 on the device, cfg, ref dict) computed once per (shape, kind)"""
    shape = _shapes()[name]
    b, cin, cout, h, w, (kh, kw), stride, padding, dilation, groups, dg = shape
    kk = kh * kw
    g = torch.Generator().manual_seed(sum(map(ord, name)) + (0 if kind == 'exact' else 100))
    base_h, base_w, ho, wo = _base_positions(shape)
    if kind == 'exact':
        x = torch.randint(-3, 4, (b, cin, h, w), generator=g).float()
        weight = torch.randint(-2, 3, (cout, cin // groups, kh, kw), generator=g).float()
        gout = torch.randint(-2, 3, (b, cout, ho, wo), generator=g).float()
        off = torch.randint(-4, 5, (b, dg, kk, 2, ho, wo), generator=g).float() * 0.5          # 0, +-0.5, +-1, +-1.5, +-2
        # planted positions: exactly -1, -0.5, H - 1, H - 0.5, H (and the same in w), and offsets of +-1e4
        for axis, size, base in ((0, h, base_h), (1, w, base_w)):
            targets = torch.tensor([-1.0, -0.5, size - 1.0, size - 0.5, float(size)])
            pick = torch.randint(0, 5, (b, dg, kk, ho, wo), generator=g)
            plant = torch.rand((b, dg, kk, ho, wo), generator=g) < 0.15
            off[:, :, :, axis] = torch.where(plant, targets[pick] - base.float(), off[:, :, :, axis])
            far = torch.rand((b, dg, kk, ho, wo), generator=g) < 0.02
            sign = torch.where(torch.rand((b, dg, kk, ho, wo), generator=g) < 0.5, -1e4, 1e4)
            off[:, :, :, axis] = torch.where(far, sign, off[:, :, :, axis])
        if name == 'a':     # every planted position at least once, whatever the draw
            for n, t in enumerate((-1.0, -0.5, h - 1.0, h - 0.5, float(h))):
                off[0, 0, n % kk, 0, n % ho, n % wo] = t - float(base_h[n % kk, n % ho, n % wo])
            for n, t in enumerate((-1.0, -0.5, w - 1.0, w - 0.5, float(w))):
                off[1, 0, n % kk, 1, n % ho, (n + 1) % wo] = t - float(base_w[n % kk, n % ho, (n + 1) % wo])
            off[1, 0, 0, 0, 0, 0], off[0, 0, 1, 1, 0, 0] = 1e4, -1e4
    else:
        x = torch.randn((b, cin, h, w), generator=g)
        weight = torch.randn((cout, cin // groups, kh, kw), generator=g)
        gout = torch.randn((b, cout, ho, wo), generator=g)
        off = torch.randn((b, dg, kk, 2, ho, wo), generator=g) * 2.0
    offset = off.reshape(b, dg * 2 * kk, ho, wo)
    x, offset, weight, gout = (t.to(DEV).contiguous() for t in (x, offset, weight, gout))
    cfg = _cfg(shape)
    out, a, gather = R.forward(x, offset, weight, **cfg)
    ref = R.backward(x, offset, weight, gout, gather=gather, **cfg)
    ref.update(out=out, a_out=a)
    return x, offset, weight, gout, cfg, ref


def _run(x, offset, weight, gout, cfg):
    import sst_amd
    x, offset, weight = (t.detach().clone().requires_grad_() for t in (x, offset, weight))
    out = sst_amd.deform_conv2d(x, offset, weight, **cfg)
    out.backward(gout)
    return dict(out=out.detach(), gin=x.grad, goff=offset.grad, gw=weight.grad)


def _k(shape):
    b, cin, cout, h, w, (kh, kw), stride, padding, dilation, groups, dg = shape
    ho, wo = R.out_size(h, w, (kh, kw), stride, padding, dilation)
    return dict(out=cin // groups * kh * kw, gin=cout // groups, goff=cin // dg + cout // groups, gw=b * ho * wo)


A_OF = dict(out='a_out', gin='a_in', goff='a_off', gw='a_w')


def test_shape_e_gives_a_block_a_second_tile():
    import sst_amd
    b, _, _, h, w, *_ = _shapes()['e']
    tiles = b * -(-h * w // sst_amd.deform_conv_tile_pixels())
    blocks = sst_amd.deform_conv_wgrad_blocks(tiles)
    assert blocks == torch.cuda.get_device_properties(0).multi_processor_count and tiles > blocks
    assert (h * w) % sst_amd.deform_conv_tile_pixels() != 0       # and the last tile is a partial one


@pytest.mark.parametrize('name', SHAPES)
def test_exact_operands_equal_the_restatement(name):
    x, offset, weight, gout, cfg, ref = _case(name, 'exact')
    # what the draw was made to contain
    shape = _shapes()[name]
    pos_h = (offset.reshape(shape[0], shape[10], -1, 2, *offset.shape[2:])[:, :, :, 0].cpu() + _base_positions(shape)[0])
    if name in ('a', 'b', 'e'):
        h = shape[3]
        for t in (-1.0, -0.5, h - 1.0, h - 0.5, float(h)):
            assert bool((pos_h == t).any()), t
        assert bool((offset == 1e4).any()) and bool((offset == -1e4).any())
    got = _run(x, offset, weight, gout, cfg)
    for key in ('out', 'gin', 'goff', 'gw'):
        want = ref[key]
        assert torch.equal(want.float().double(), want), f'{key}: the restatement is not exact in fp32 - the operands are too large'
        assert bool(torch.isfinite(got[key]).all())
        diff = (got[key].double() - want).abs()
        assert torch.equal(got[key], want.float()), f'{name} {key}: {int((diff > 0).sum())} elements differ, max {float(diff.max())}'
    assert float(ref['gin'].abs().max()) > 0 and float(ref['goff'].abs().max()) > 0 and float(ref['gw'].abs().max()) > 0


@pytest.mark.parametrize('name', SHAPES)
def test_general_operands_stay_within_the_derived_bound(name):
    x, offset, weight, gout, cfg, ref = _case(name, 'general')
    shape = _shapes()[name]
    got = _run(x, offset, weight, gout, cfg)
    # offsets within 1e-3 of an integer (the position is the offset plus an integer: cell and border changes sit there)
    b, dg = shape[0], shape[10]
    off = offset.reshape(b, dg, -1, 2, *offset.shape[2:])
    near = ((off - off.round()).abs() < 1e-3).any(3, keepdim=True).expand_as(off).reshape(offset.shape)
    assert float(near.float().mean()) <= 0.01
    for key, k in _k(shape).items():
        err = (got[key].double() - ref[key]).abs()
        bound = (k + 16) * EPS * ref[A_OF[key]]
        ratio = err / bound.clamp_min(1e-300)
        print(f'{name} {key}: K = {k}, max err / bound = {float(ratio.max()):.4f}')
        if key == 'goff':
            ratio = torch.where(near, torch.zeros_like(ratio), ratio)
        assert bool(torch.isfinite(got[key]).all())
        assert float(ratio.max()) <= 1.0, f'{name} {key}: err / bound = {float(ratio.max())}'


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd70'])
def test_zero_offsets_are_conv2d(name):
    import sst_amd
    x, offset, weight, gout, cfg, _ = _case(name, 'general')
    shape = _shapes()[name]
    out = sst_amd.deform_conv2d(x, torch.zeros_like(offset), weight, **cfg)
    want = F.conv2d(x.double(), weight.double(), None, cfg['stride'], cfg['padding'], cfg['dilation'], cfg['groups'])
    a = F.conv2d(x.double().abs(), weight.double().abs(), None, cfg['stride'], cfg['padding'], cfg['dilation'], cfg['groups'])
    assert out.shape == want.shape
    assert bool(((out.double() - want).abs() <= (_k(shape)['out'] + 16) * EPS * a).all())
    # and equal to the convolution where every operand is a small integer
    x, offset, weight, _, cfg, _ = _case(name, 'exact')
    out = sst_amd.deform_conv2d(x, torch.zeros_like(offset), weight, **cfg)
    assert torch.equal(out.double(), F.conv2d(x.double(), weight.double(), None, cfg['stride'], cfg['padding'], cfg['dilation'],
                                              cfg['groups']))


@pytest.mark.parametrize('name', ['b', 'e'])
def test_two_runs_are_bit_identical(name):
    x, offset, weight, gout, cfg, _ = _case(name, 'general')
    first, second = _run(x, offset, weight, gout, cfg), _run(x, offset, weight, gout, cfg)
    for key in first:
        assert torch.equal(first[key].view(torch.int32), second[key].view(torch.int32)), key


def test_no_column_buffer_is_allocated():
    """B 1, 16 -> 16, 64 x 64: the column buffer would be 9 x either tensor"""
    import sst_amd
    g = torch.Generator().manual_seed(5)
    x = torch.randn((1, 16, 64, 64), generator=g).to(DEV).requires_grad_()
    offset = (torch.randn((1, 18, 64, 64), generator=g) * 2).to(DEV).requires_grad_()
    weight = torch.randn((16, 16, 3, 3), generator=g).to(DEV).requires_grad_()
    gout = torch.randn((1, 16, 64, 64), generator=g).to(DEV)
    sst_amd.deform_conv2d(x, offset, weight, padding=1).backward(gout)      # the library is loaded, the allocator warm
    x.grad = offset.grad = weight.grad = None
    torch.cuda.synchronize()
    in_bytes, off_bytes, out_bytes = x.numel() * 4, offset.numel() * 4, gout.numel() * 4
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = sst_amd.deform_conv2d(x, offset, weight, padding=1)
    torch.cuda.synchronize()
    fwd_peak = torch.cuda.max_memory_allocated() - base
    print(f'forward peak above the inputs: {fwd_peak} bytes, output {out_bytes}')
    assert fwd_peak <= 1.25 * out_bytes
    base = torch.cuda.memory_allocated()           # inputs, output and gout
    torch.cuda.reset_peak_memory_stats()
    out.backward(gout)
    torch.cuda.synchronize()
    bwd_peak = torch.cuda.max_memory_allocated() - base
    print(f'backward peak above inputs + gout: {bwd_peak} bytes, bound {4 * in_bytes + off_bytes + (1 << 20)}')
    assert bwd_peak <= 4 * in_bytes + off_bytes + (1 << 20)
    assert x.grad is not None and offset.grad is not None and weight.grad is not None


def test_refusals_on_the_device():
    import sst_amd
    x = torch.zeros(1, 4, 5, 5, device=DEV)
    with pytest.raises(RuntimeError, match='fp32 tensors only'):
        sst_amd.deform_conv2d(x.half(), torch.zeros(1, 18, 5, 5, device=DEV).half(), torch.zeros(4, 4, 3, 3, device=DEV).half(),
                              padding=1)
    with pytest.raises(NotImplementedError, match='above 3 x 3'):
        sst_amd.deform_conv2d(x, torch.zeros(1, 50, 5, 5, device=DEV), torch.zeros(4, 4, 5, 5, device=DEV), padding=2)
    with pytest.raises(RuntimeError, match='offset must be'):
        sst_amd.deform_conv2d(x, torch.zeros(1, 18, 4, 5, device=DEV), torch.zeros(4, 4, 3, 3, device=DEV), padding=1)
    with pytest.raises(RuntimeError, match='must divide'):
        sst_amd.deform_conv2d(x, torch.zeros(1, 18, 5, 5, device=DEV), torch.zeros(4, 4, 3, 3, device=DEV), padding=1, groups=3)
