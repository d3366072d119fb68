"""The fused SIR stage without a GPU: the C ABI declares it, the package exports it, the switch reaches every SIRLayer and keeps
the parameter names, and the split-weight identity the second stage relies on holds."""
import os
import re

import pytest
import torch

from conftest import ROOT, load_golden


def _sir():
    import sst_amd
    return sst_amd.build_backbone(dict(type='SIR', num_blocks=3, in_channels=[84, 133, 133],
                                       feat_channels=[[128, 128]] * 3, rel_mlp_hidden_dims=[[16, 32]] * 3,
                                       norm_cfg=dict(type='LN', eps=1e-3), mode='max', xyz_normalizer=[20, 20, 4],
                                       act='gelu', unique_once=True))


def test_header_declares_the_stage_entry_points():
    text = open(os.path.join(ROOT, 'include', 'sst_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    names = set(re.findall(r'\b(sst_[a-z0-9_]+)\s*\(', text))
    assert 'sst_sir_gather_segmax_fwd_f32' in names
    assert 'sst_sir_gather_segmax_bwd_f32' in names


def test_package_exports_the_stage_and_the_switch():
    import sst_amd
    assert callable(sst_amd.sir_stage) and callable(sst_amd.enable_fused_sir) and callable(sst_amd.sir_stage_ok)
    from sst_amd import _lib
    assert 'sst_sir_gather_segmax_fwd_f32' in _lib.EXPORTED_SYMBOLS and 'sst_sir_gather_segmax_bwd_f32' in _lib.EXPORTED_SYMBOLS


def test_sir_stage_refuses_cpu_tensors():
    import sst_amd
    from sst_amd import kernels as K
    plan = K.UniquePlan()
    plan.n, plan.m = 8, 2
    norm = torch.nn.LayerNorm(128, eps=1e-3)
    with pytest.raises(RuntimeError):
        sst_amd.sir_stage(torch.zeros(8, 84), torch.zeros(128, 84), norm, None, plan)
    with pytest.raises(RuntimeError):
        sst_amd.sir_stage(torch.zeros(8, 128), torch.zeros(128, 128), norm, torch.nn.ReLU(), plan, add_rows=torch.zeros(2, 128))


def test_the_switch_is_off_by_default_and_reaches_every_layer():
    import sst_amd
    sir = _sir()
    layers = [m for m in sir.modules() if isinstance(m, sst_amd.SIRLayer)]
    assert len(layers) == 3
    assert all(m.fused_stage is False for m in layers)
    assert sst_amd.enable_fused_sir(sir) is sir
    assert all(m.fused_stage is True for m in layers)
    sst_amd.enable_fused_sir(sir, False)
    assert all(m.fused_stage is False for m in layers)
    one = layers[0]
    sst_amd.enable_fused_sir(one)          # a SIRLayer itself is "below" itself
    assert one.fused_stage is True and layers[1].fused_stage is False


def test_golden_weights_load_strictly_with_the_switch_on():
    import sst_amd
    g = load_golden('sir.npz')
    sir = sst_amd.enable_fused_sir(_sir())
    before = list(sir.state_dict().keys())
    sd = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith('w::')}
    sir.load_state_dict(sd, strict=True)
    assert list(sir.state_dict().keys()) == before == list(_sir().state_dict().keys())


def test_split_weight_identity_in_float64():
    """cat([y, pooled[inv]]) W^T == y W[:, :128]^T + (pooled W[:, 128:]^T)[inv]: what lets the second stage skip the [N, 256] matrix"""
    g = torch.Generator().manual_seed(11)
    n, m = 500, 37
    inv = torch.randint(0, m, (n,), generator=g)
    y = torch.randn(n, 128, generator=g, dtype=torch.float64)
    pooled = torch.randn(m, 128, generator=g, dtype=torch.float64)
    w = torch.randn(128, 256, generator=g, dtype=torch.float64) / 16
    whole = torch.cat([y, pooled[inv]], dim=1) @ w.t()
    split = y @ w[:, :128].t() + (pooled @ w[:, 128:].t())[inv]
    assert float((whole - split).abs().max()) <= 1e-12
