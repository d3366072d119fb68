"""Host side of the 'bf16' operand mode of the sparse convolutions (no GPU): the per-module precision switch, the fp16 contract
of the sparse U-Nets (_lib.Fp32Master), the host-only library calls of csrc/spconv_os_bf16.hip, and the exactness condition of
recipe E (tests/spconv_bf16_ref.py) for every shape tests/test_gpu_spconv_bf16.py uses."""
import inspect

import pytest
import torch

import spconv_bf16_ref as B
import spconv_exact_ref as R

# the backbone of configs/fsd/fsd_waymoD1_1x.py:39-51 (as tests/test_gpu_sparse_unet.py restates it)
FSD_UNET = dict(
    type='SimpleSparseUNet', in_channels=64, sparse_shape=[32, 640, 640], order=('conv', 'norm', 'act'),
    norm_cfg=dict(type='naiveSyncBN1d', eps=1e-3, momentum=0.01), base_channels=64, output_channels=128,
    encoder_channels=((64, ), (64, 64, 64), (64, 64, 64), (128, 128, 128), (256, 256, 256)),
    encoder_paddings=((1, ), (1, 1, 1), (1, 1, 1), ((0, 1, 1), 1, 1), (1, 1, 1)),
    decoder_channels=((256, 256, 128), (128, 128, 64), (64, 64, 64), (64, 64, 64), (64, 64, 64)),
    decoder_paddings=((1, 1), (1, 0), (1, 0), (0, 0), (0, 1)))


def _convs(module):
    from sst_amd import spconv
    return [m for m in module.modules() if isinstance(m, spconv.SparseConvolution)]


def test_module_precision_switch():
    """SparseConvolution.set_precision takes None, 'f32', 'f32x3', 'f32x6', 'bf16' and nothing else; the default is None; the
    U-Net's set_precision and set_module_precision reach every convolution of FSD's SimpleSparseUNet"""
    import sst_amd
    from sst_amd import spconv
    conv = spconv.SubMConv3d(8, 8, 3, padding=1, bias=False)
    assert conv.precision is None and spconv.SparseConvolution.precision is None
    for mode in (None, 'f32', 'f32x3', 'f32x6', 'bf16'):
        assert conv.set_precision(mode) is conv and conv.precision == mode
    for bad in ('fp16', 'bf16 ', 'BF16', 16, 'f32x2', ''):
        with pytest.raises(ValueError):
            conv.set_precision(bad)
    assert conv.precision == 'bf16'
    net = sst_amd.BACKBONES.build(dict(FSD_UNET))
    convs = _convs(net)
    assert len(convs) == 1 + 13 + 5 * 4 and all(c.precision is None for c in convs)      # input, encoder, 4 per decoder level
    assert net.set_precision('bf16') is net and all(c.precision == 'bf16' for c in convs)
    assert net.set_precision(None) is net and all(c.precision is None for c in convs)
    holder = torch.nn.ModuleDict(dict(segmentor=torch.nn.Sequential(torch.nn.Linear(2, 2), net)))
    assert spconv.set_module_precision(holder, 'bf16') is holder and all(c.precision == 'bf16' for c in convs)
    with pytest.raises(ValueError):
        spconv.set_module_precision(holder, 'half')
    with pytest.raises(ValueError):
        net.set_precision('half')
    assert all(c.precision == 'bf16' for c in convs)
    # a module made afterwards is untouched: the mode is per module
    assert spconv.SubMConv3d(8, 8, 3).precision is None


def test_global_switch_is_untouched_and_still_rejects_bf16():
    import sst_amd
    from sst_amd import spconv
    before = spconv.conv_precision()
    sst_amd.BACKBONES.build(dict(FSD_UNET)).set_precision('bf16')
    spconv.SubMConv3d(4, 4, 3).set_precision('bf16')
    assert spconv.conv_precision() == before == spconv.DEFAULT_CONV_PRECISION
    with pytest.raises(ValueError):
        spconv.set_conv_precision('bf16')
    assert spconv.conv_precision() == before
    for fn in (spconv._gather_gemm, spconv._wgrad, spconv.indice_conv, spconv.indice_conv_backward):
        assert inspect.signature(fn).parameters['precision'].default is None


def test_host_only_library_calls():
    """the workspace of the bf16 rows entry: positive, smaller than the x6 entry's (2 bytes per packed weight instead of 6);
    the plan query answers for the new entry code; both reject sizes that are not positive"""
    from sst_amd import _lib
    lib = _lib.load()
    for kvol, cin, cout, m in ((27, 64, 64, 130), (27, 16, 32, 2000), (27, 128, 160, 70000), (1, 4, 4, 1), (32, 256, 256, 300000),
                               (8, 68, 132, 6000)):
        mine = lib.sst_spconv_conv_os_bf16_workspace_bytes_rows(kvol, cin, cout, m)
        x6 = lib.sst_spconv_conv_os_f32x6_workspace_bytes_rows(kvol, cin, cout, m)
        assert 0 < mine < x6, (kvol, cin, cout, m, mine, x6)
        pack = lib.sst_spconv_conv_os_bf16_workspace_bytes_rows(kvol, cin, cout, 0)
        assert 0 < pack <= mine and pack % 256 == 0
        rc, rows, cols, split, wgs = R.conv_plan(B.ROWS_BF16, m, kvol, cin, cout, 0, mine)
        assert rc == 0 and rows == 64 and cols in (64, 128) and split in (1, 2, 4, 8) and (split == 1 or split <= kvol)
        live = -(-m // rows) * -(-cout // cols) * split
        assert live <= wgs < live + 32 and wgs % 8 == 0
        assert (mine == pack) == (split == 1)
        assert R.conv_plan(B.ROWS_BF16, m, kvol, cin, cout, 0, pack)[3] == 1          # nowhere to put partial tiles
        assert R.conv_plan(B.ROWS_BF16, m, kvol, cin, cout, 0, pack - 1)[0] == _lib.SST_ERR_ARG
    assert R.conv_plan(B.ROWS_BF16, 130, 27, 64, 64, 0, 1 << 30)[3] > 1                # a thin level is split
    for bad in ((0, 8, 8, 10), (27, 0, 8, 10), (27, 8, 0, 10), (27, 8, 8, -1), (-1, 8, 8, 10)):
        assert lib.sst_spconv_conv_os_bf16_workspace_bytes_rows(*bad) == _lib.SST_ERR_ARG, bad
    for m, kvol, cin, cout in ((0, 27, 8, 8), (10, 0, 8, 8), (10, 27, 0, 8), (10, 27, 8, 0), (-3, 27, 8, 8)):
        assert R.conv_plan(B.ROWS_BF16, m, kvol, cin, cout, 0, 1 << 30)[0] == _lib.SST_ERR_ARG
    assert R.conv_plan(B.ROWS_BF16, 100, 27, 6, 16, 0, 1 << 30)[0] == _lib.SST_ERR_UNSUPPORTED
    assert R.conv_plan(B.ROWS_BF16, 100, 33, 8, 16, 0, 1 << 30)[0] == _lib.SST_ERR_UNSUPPORTED
    assert R.conv_plan(B.ROWS_BF16, 100, 27, 8, 16, 41, 1 << 30)[0] == _lib.SST_ERR_ARG


def test_half_keeps_the_fp32_masters_of_the_sparse_unets():
    """`model.half()` on the three U-Net backbones: remembered, not applied - every parameter and buffer stays fp32 and
    wants_half is true (on the parent commit they became half and the first forward raised)"""
    import sst_amd
    from sst_amd import _lib
    small = dict(in_channels=8, sparse_shape=[16, 40, 40], base_channels=16, output_channels=24,
                 encoder_channels=((16, ), (16, 16), (16, 16)), encoder_paddings=((1, ), (1, 1), (1, 1)),
                 decoder_channels=((16, 16, 16), (16, 16, 16), (16, 16, 16)), decoder_paddings=((1, 1), (1, 1), (1, 1)))
    for net in (sst_amd.BACKBONES.build(dict(FSD_UNET)), sst_amd.VirtualVoxelMixer(**small), sst_amd.SparseUNet(**small)):
        assert isinstance(net, _lib.Fp32Master) and not net.half_requested and not _lib.wants_half(net)
        assert net.half() is net and net.half_requested and _lib.wants_half(net)
        assert all(p.dtype == torch.float32 for p in net.parameters())
        assert all(b.dtype != torch.float16 for b in net.buffers()) and len(list(net.buffers())) > 0
        assert all(c.precision is None for c in _convs(net))            # the request is not an explicit precision
    # below a parent that is not one of ours
    net = sst_amd.SimpleSparseUNet(**small)
    parent = torch.nn.Sequential(torch.nn.Linear(4, 4), net).half()
    assert parent[0].weight.dtype == torch.float16 and all(p.dtype == torch.float32 for p in net.parameters())
    assert _lib.wants_half(net)
    # other conversions apply
    assert all(p.dtype == torch.float64 for p in net.double().parameters())
    assert all(p.dtype == torch.float32 for p in net.float().parameters())


def test_recipe_e_is_exact_for_every_gpu_shape():
    """E uses all 8 significand bits of bf16 and nothing beyond them; its worst-case sums stay below the exactness limit for
    every (kvol, channels) of the GPU tests and for the longest pair list of the filter-gradient tests"""
    gen = torch.Generator().manual_seed(1)
    fine = B.values('E', True, (100000,), gen)
    unit = B.values('E', False, (1000,), gen)
    assert B.is_bf16(fine) and B.is_bf16(unit) and B.is_bf16(B.values('A', True, (1000,), gen))
    assert float(fine.abs().max()) == 255 / 128 and set(unit.tolist()) == {-1.0, 0.0, 1.0}
    k = (fine * 128).abs().long()
    assert bool((k >= 129).any()) and bool((k % 2 == 1).any())          # 8-bit significands with the last bit set
    assert not B.is_bf16(torch.tensor([1 + 2.0 ** -8])) and B.round_bf16(torch.tensor([1 + 2.0 ** -8])).item() == 1.0
    assert max(kv for kv, _ in B.GPU_CONV_SHAPES) <= 32 and max(c for _, c in B.GPU_CONV_SHAPES) <= 256
    for kvol, c in B.GPU_CONV_SHAPES:
        assert B.worst_case_granules(kvol, c) + 255 < R.LIMIT, (kvol, c)           # + a bias of the fine kind
        x = torch.full((3, c), 255 / 128)
        w = torch.ones(kvol, c, 5)
        mp = torch.zeros(kvol, 4, dtype=torch.int32)
        R.assert_conv_exact('E', x, mp, w, torch.full((5,), 255 / 128))
    assert B.worst_case_granules(B.GPU_WGRAD_MAX_PAIRS, 1) < R.LIMIT
    with pytest.raises(AssertionError):
        R.assert_exact('E', torch.tensor([float(R.LIMIT) * B.GRANULE_E]))
