"""The deformable convolution without a GPU: the float64 restatement (tests/deform_conv_ref.py) against the two identities that
need no other implementation (zero offsets = F.conv2d, integer offsets = a convolution of shifted zero-padded input) and against
gradcheck; the Python surface (deform_conv2d, DeformConv2d, DeformConv2dPack, build_conv_layer 'DCN', the refusals); the keys and
shapes of CenterHead's network after attach_network(); the keys DynamicVoxelNet / DynamicCenterPoint gain from attach_heads()."""
import ast
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT

import deform_conv_ref as R

CENTER_CONFIGS = ('sst_waymoD5_1x_3class_centerhead', 'sst_waymoD1_2x_3class_centerhead')

# (B, Cin, Cout, H, W, kernel, stride, padding, dilation, groups, deform_groups)
CASES = {
    'k3p1': (2, 8, 8, 5, 7, (3, 3), 1, 1, 1, 1, 1),
    'groups': (1, 12, 20, 9, 10, (3, 3), 2, 2, 2, 2, 2),
    'k1': (2, 6, 4, 1, 9, (1, 1), 1, 0, 1, 1, 3),
    'k23': (1, 4, 6, 6, 5, (2, 3), (1, 2), (1, 0), (2, 1), 2, 1),
}


def _operands(case, seed=0):
    b, cin, cout, h, w, kernel, stride, padding, dilation, groups, dg = CASES[case]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, cin, h, w, generator=g, dtype=torch.float64)
    weight = torch.randn(cout, cin // groups, *kernel, generator=g, dtype=torch.float64)
    ho, wo = R.out_size(h, w, kernel, stride, padding, dilation)
    cfg = dict(stride=stride, padding=padding, dilation=dilation, groups=groups, deform_groups=dg)
    return x, weight, (b, dg * 2 * kernel[0] * kernel[1], ho, wo), cfg, g


@pytest.mark.parametrize('case', list(CASES))
def test_zero_offsets_are_a_convolution(case):
    x, weight, off_shape, cfg, _ = _operands(case)
    out, a, _ = R.forward(x, torch.zeros(off_shape, dtype=torch.float64), weight, **cfg)
    want = F.conv2d(x, weight, None, cfg['stride'], cfg['padding'], cfg['dilation'], cfg['groups'])
    assert out.shape == want.shape
    assert bool(((out - want).abs() <= 1e-14 * a + 1e-300).all())
    assert bool((a >= out.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize('case', ['k3p1', 'groups', 'k23'])
def test_integer_offsets_are_a_convolution_of_shifted_input(case):
    x, weight, off_shape, cfg, g = _operands(case)
    b, cin, cout, h, w, kernel, *_ = CASES[case]
    assert cfg['deform_groups'] in (1, 2)
    kk = kernel[0] * kernel[1]
    # one (a, b) per tap, the same at every pixel and in every deformable group; shifts past the image included
    shifts = [(int(torch.randint(-h - 1, h + 2, (1,), generator=g)), int(torch.randint(-3, 4, (1,), generator=g))) for _ in range(kk)]
    offset = torch.zeros(off_shape, dtype=torch.float64)
    for d in range(cfg['deform_groups']):
        for k, (a_, b_) in enumerate(shifts):
            offset[:, d * 2 * kk + 2 * k], offset[:, d * 2 * kk + 2 * k + 1] = a_, b_
    out, a, _ = R.forward(x, offset, weight, **cfg)
    want = R.shifted_conv(x, weight, shifts, cfg['stride'], cfg['padding'], cfg['dilation'], cfg['groups'])
    assert bool(((out - want).abs() <= 1e-14 * a + 1e-300).all())
    assert float(out.abs().max()) > 0


def _smooth_offsets(shape, g, spread=2.0, margin=0.05):
    """offsets whose positions stay ``margin`` clear of the integers (hence of the -1 / H borders, which are integers)"""
    off = torch.randn(shape, generator=g, dtype=torch.float64) * spread
    frac = off - torch.floor(off)
    return torch.floor(off) + frac.clamp(margin, 1 - margin)


@pytest.mark.parametrize('case', list(CASES))
def test_analytic_gradients_pass_gradcheck(case):
    x, weight, off_shape, cfg, g = _operands(case, seed=3)
    offset = _smooth_offsets(off_shape, g)          # integer strides, paddings and dilations: the position is off + an integer
    x, offset, weight = (t.requires_grad_() for t in (x, offset, weight))
    assert torch.autograd.gradcheck(lambda a, b, c: R.RefDeformConv.apply(a, b, c, cfg), (x, offset, weight), eps=1e-6, atol=1e-7,
                                    rtol=1e-6)


def test_the_surface_exists():
    import sst_amd
    assert callable(sst_amd.deform_conv2d)
    layer = sst_amd.build_conv_layer(dict(type='DCN', in_channels=64, out_channels=64, kernel_size=3, padding=1, groups=4,
                                          bias=False))
    assert isinstance(layer, sst_amd.DeformConv2dPack) and isinstance(layer, sst_amd.DeformConv2d)
    state = layer.state_dict()
    assert {k: tuple(v.shape) for k, v in state.items()} == {'weight': (64, 16, 3, 3), 'conv_offset.weight': (18, 64, 3, 3),
                                                            'conv_offset.bias': (18,)}
    assert not state['conv_offset.weight'].any() and not state['conv_offset.bias'].any() and state['weight'].any()
    assert layer.conv_offset.padding == (1, 1) and layer.conv_offset.kernel_size == (3, 3)
    two = sst_amd.DeformConv2dPack(8, 12, (2, 3), stride=2, padding=1, dilation=1, groups=2, deform_groups=4)
    assert tuple(two.conv_offset.weight.shape) == (4 * 2 * 6, 8, 2, 3) and tuple(two.weight.shape) == (12, 4, 2, 3)
    # the four types the function built before
    assert isinstance(sst_amd.build_conv_layer(None, 4, 4, 1), torch.nn.Conv2d)
    assert isinstance(sst_amd.build_conv_layer(dict(type='Conv1d'), 4, 4, 1), torch.nn.Conv1d)
    assert isinstance(sst_amd.build_conv_layer(dict(type='Conv3d'), 4, 4, 1), torch.nn.Conv3d)
    assert isinstance(sst_amd.build_conv_layer(dict(type='Conv'), 4, 4, 1), torch.nn.Conv2d)
    with pytest.raises(KeyError):
        sst_amd.build_conv_layer(dict(type='NoSuchConv'), 4, 4, 1)
    import sst_amd.native_shims as shims
    assert shims.mmcv_deform_conv.DeformConv2dPack is sst_amd.DeformConv2dPack and callable(shims.mmcv_deform_conv.deform_conv2d)


def test_symbols_are_in_the_header_and_the_library():
    from sst_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sst_amd.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(sst_deform_conv_[a-z0-9_]+)\s*\(', text))
    assert {'sst_deform_conv_fwd_f32', 'sst_deform_conv_bwd_f32', 'sst_deform_conv_bwd_workspace_bytes',
            'sst_deform_conv_tile_pixels'} <= declared
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, name) for name in declared)
    import sst_amd
    assert sst_amd.deform_conv_tile_pixels() >= 32
    # shapes are checked on the host: a 5 x 5 kernel and a group count that does not divide are refused by the library itself
    shape = _lib.DeformConvShape(1, 8, 9, 9, 8, 5, 5, 1, 1, 2, 2, 1, 1, 1, 1, 0)
    assert _lib.load().sst_deform_conv_fwd_f32(ctypes.byref(shape), None, None, None, None, None) == _lib.SST_ERR_UNSUPPORTED
    shape = _lib.DeformConvShape(1, 8, 9, 9, 8, 3, 3, 1, 1, 1, 1, 1, 1, 3, 1, 0)
    assert _lib.load().sst_deform_conv_fwd_f32(ctypes.byref(shape), None, None, None, None, None) == _lib.SST_ERR_ARG


def test_cpu_tensors_raise():
    import sst_amd
    x, off, w = torch.zeros(1, 4, 5, 5), torch.zeros(1, 18, 5, 5), torch.zeros(4, 4, 3, 3)
    with pytest.raises(RuntimeError, match='no CPU path'):
        sst_amd.deform_conv2d(x, off, w, padding=1)
    with pytest.raises(RuntimeError, match='no CPU path'):
        sst_amd.DeformConv2d(4, 4, 3, padding=1)(x, off)
    with pytest.raises(RuntimeError, match='no CPU path'):
        sst_amd.DeformConv2dPack(4, 4, 3, padding=1)(x)


def test_unsupported_variants_are_refused_by_name():
    import sst_amd
    with pytest.raises(NotImplementedError, match='DCNv2'):
        sst_amd.build_conv_layer(dict(type='DCNv2', in_channels=4, out_channels=4, kernel_size=3, padding=1))
    with pytest.raises(NotImplementedError, match='bias=True'):
        sst_amd.build_conv_layer(dict(type='DCN', in_channels=4, out_channels=4, kernel_size=3, padding=1, bias=True))
    with pytest.raises(NotImplementedError, match='above 3 x 3'):
        sst_amd.DeformConv2dPack(4, 4, 5, padding=2)
    with pytest.raises(NotImplementedError, match='above 3 x 3'):
        sst_amd.DeformConv2d(4, 4, (1, 4))
    for dtype in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(RuntimeError, match='fp32 tensors only'):
            sst_amd.deform_conv2d(torch.zeros(1, 4, 5, 5, dtype=dtype), torch.zeros(1, 18, 5, 5, dtype=dtype),
                                  torch.zeros(4, 4, 3, 3, dtype=dtype), padding=1)


def _model_cfg(name):
    return ast.literal_eval(open(os.path.join(GOLDEN, 'configs', 'sst_refactor', name + '.model.py')).read())


def _bn(prefix, c):
    return {f'{prefix}.weight': (c,), f'{prefix}.bias': (c,), f'{prefix}.running_mean': (c,), f'{prefix}.running_var': (c,),
            f'{prefix}.num_batches_tracked': ()}


@pytest.mark.parametrize('name', CENTER_CONFIGS)
def test_center_head_network_has_the_reference_keys(name):
    import sst_amd
    model = _model_cfg(name)
    cfg = dict(model['bbox_head'], train_cfg=model['train_cfg'], test_cfg=model['test_cfg'])
    head = sst_amd.build_head(cfg)
    assert not hasattr(head, 'attach_network') or not list(head.parameters())
    unbuilt = {k: v for k, v in head.unbuilt.items()}
    assert head.attach_network() is head
    assert head.unbuilt == unbuilt == {k: head.unbuilt[k] for k in unbuilt}
    want = {'shared_conv.conv.weight': (64, 128, 3, 3), **_bn('shared_conv.bn', 64)}
    t = 'task_heads.0.'
    for adapt in ('feature_adapt_cls', 'feature_adapt_reg'):
        want.update({f'{t}{adapt}.weight': (64, 16, 3, 3), f'{t}{adapt}.conv_offset.weight': (18, 64, 3, 3),
                     f'{t}{adapt}.conv_offset.bias': (18,)})
    want.update({f'{t}cls_head.0.conv.weight': (64, 64, 3, 3), **_bn(f'{t}cls_head.0.bn', 64),
                 f'{t}cls_head.1.weight': (3, 64, 3, 3), f'{t}cls_head.1.bias': (3,)})
    for head_name, c in (('reg', 2), ('height', 1), ('dim', 3), ('rot', 2), ('vel', 2)):
        p = f'{t}task_head.{head_name}'
        want.update({f'{p}.0.conv.weight': (64, 64, 3, 3), **_bn(f'{p}.0.bn', 64), f'{p}.1.weight': (c, 64, 3, 3),
                     f'{p}.1.bias': (c,)})
    got = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    assert got == want
    state = head.state_dict()
    for adapt in ('feature_adapt_cls', 'feature_adapt_reg'):
        assert not state[f'{t}{adapt}.conv_offset.weight'].any() and not state[f'{t}{adapt}.conv_offset.bias'].any()
    assert bool((state[f'{t}cls_head.1.bias'] == torch.tensor(-2.19)).all())
    assert isinstance(head.shared_conv.bn, sst_amd.NaiveSyncBatchNorm2d) and head.shared_conv.bn.eps == 1e-3
    # circle NMS stays refused
    head.test_cfg = dict(head.test_cfg, nms_type='circle')
    with pytest.raises(NotImplementedError, match='circle'):
        head.get_bboxes([[dict()]], [dict()])


@pytest.mark.parametrize('name', CENTER_CONFIGS + ('sst_waymoD5_1x_3class_8heads_v2',))
def test_attach_heads_adds_the_neck_and_the_head(name):
    import sst_amd
    model = _model_cfg(name)
    torch.manual_seed(0)
    plain = sst_amd.build_detector(model)
    before = {k: tuple(v.shape) for k, v in plain.state_dict().items()}
    assert before and not any(k.startswith(('neck.', 'bbox_head.')) for k in before)
    for step in (plain.forward_train, plain.simple_test, plain.aug_test):
        with pytest.raises(NotImplementedError):
            step([], [], [], [])
    det = sst_amd.build_detector(model)
    unbuilt = dict(det.unbuilt)
    assert det.attach_heads() is det and det.with_neck and not plain.with_neck
    assert det.unbuilt == unbuilt == {k: model[k] for k in ('neck', 'bbox_head')}
    after = {k: tuple(v.shape) for k, v in det.state_dict().items()}
    added = set(after) - set(before)
    assert {k: after[k] for k in before} == before
    assert added and all(k.startswith(('neck.', 'bbox_head.')) for k in added)
    assert any(k.startswith('neck.deblocks.0.0.') for k in added)
    if model['type'] == 'DynamicCenterPoint':
        assert 'bbox_head.task_heads.0.feature_adapt_cls.conv_offset.bias' in added and 'bbox_head.shared_conv.conv.weight' in added
    else:
        assert {'bbox_head.conv_cls.weight', 'bbox_head.conv_reg.weight', 'bbox_head.conv_dir_cls.weight'} <= added
    with pytest.raises(NotImplementedError, match='aug_test'):
        det.aug_test([], [])
