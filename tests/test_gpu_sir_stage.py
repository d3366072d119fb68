"""GPU: the fused SIR stage (csrc/sir_stage.hip) - structure of the pooling, the exact product, values and gradients against
float64, the routing of the pooling's gradient, the reference's golden tensors through the switch, the fall-backs."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
C = 128


# ------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------
def _plan_of_ids(ids):
    """native grouping (this library's sorted-unique) of rows by their id; every id 0..max occurs, so group g = id g"""
    from sst_amd import kernels as K
    plan = K.unique_rows(torch.as_tensor(ids, dtype=torch.int64).reshape(-1, 1).contiguous().to(DEV))
    assert plan.m == int(np.max(ids)) + 1
    return plan


def _ids_of_sizes(sizes, rng):
    ids = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(ids)
    return ids


def _small_groups(n, rng):
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(rng.integers(1, 8)))
    sizes[-1] -= sum(sizes) - n
    return [s for s in sizes if s > 0]


def _raw_fwd(x, w, gamma, beta, eps, act, plan, add_rows=None):
    """the C entry point on NaN-filled outputs (so that an unwritten element shows)"""
    from sst_amd import _lib
    from sst_amd import kernels as K
    n, k = x.shape
    m = plan.m
    nan = float('nan')
    pre = torch.full((n, C), nan, device=DEV)
    y = torch.full((n, C), nan, device=DEV)
    stats = torch.full((n, 2), nan, device=DEV)
    pooled = torch.full((m, C), nan, device=DEV)
    argmax = torch.full((m, C), -7, dtype=torch.int32, device=DEV)
    scratch = K._long_group_scratch(plan, n, m, C, x.device)
    rc = _lib.load().sst_sir_gather_segmax_fwd_f32(
        _lib.ptr(x), n, k, _lib.ptr(w), w.stride(0), w.size(0), _lib.ptr(add_rows), _lib.ptr(gamma), _lib.ptr(beta), float(eps),
        act, _lib.ptr(plan.perm), _lib.ptr(plan.inverse), _lib.ptr(plan.offsets), m, _lib.ptr(scratch), _lib.ptr(pre),
        _lib.ptr(stats), _lib.ptr(y), _lib.ptr(pooled), _lib.ptr(argmax), _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return pre, stats, y, pooled, argmax


def _group_max_and_first_row(y, ids, m):
    """float32 group maximum of y and the smallest row attaining it (CPU, exact)"""
    n, c = y.shape
    idx = torch.as_tensor(ids).view(-1, 1).expand(-1, c)
    mx = torch.full((m, c), float('-inf')).scatter_reduce(0, idx, y, reduce='amax')
    hit = y == mx[torch.as_tensor(ids)]
    cand = torch.where(hit, torch.arange(n).view(-1, 1).expand(-1, c), torch.full((n, c), n))
    first = torch.full((m, c), n, dtype=torch.long).scatter_reduce(0, idx, cand, reduce='amin')
    return mx, first


def _structure_cases():
    cases = [('n%d' % n, n) for n in (1, 15, 16, 17, 63, 64, 65, 1000)]
    return cases + [('long_groups_and_tile_edges', None)]


# ------------------------------------------------------------------------------------------------------------------
# 1. structure, exact
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,n', _structure_cases(), ids=[c[0] for c in _structure_cases()])
def test_pooling_structure_is_exact(name, n):
    """pooled == the group-wise maximum of the kernel's OWN y bit for bit, argmax == the smallest row attaining it, every row of
    y / pre / stats written.  K = 133 (rows not 16-byte aligned), ReLU (exact zeros tie everywhere)."""
    import sst_amd
    tile = sst_amd.sir_stage_tile_rows()
    rng = np.random.default_rng(7 if n is None else n)
    if n is not None:
        sizes = _small_groups(n, rng)
    else:
        sizes = np.concatenate([[3000, 1700, 512, 65, 64, 63], rng.integers(1, 40, size=700)]).astype(np.int64)
        # in sorted order group g starts at the sum of the sizes before it: make one boundary right behind the long groups and
        # one further back fall exactly on a tile edge (the group before ends on it, the group behind begins on it)
        sizes[6] = tile - int(sizes[:6].sum()) % tile
        assert 1 <= sizes[6] <= 39
        cum = np.cumsum(sizes)
        j = next(j for j in range(300, 700) if 1 <= tile - int(cum[j - 1]) % tile <= 39)
        sizes[j] = tile - int(cum[j - 1]) % tile
        cum = np.cumsum(sizes)
        assert cum[6] % tile == 0 and cum[j] % tile == 0
        sizes = list(sizes)
    ids = _ids_of_sizes(sizes, rng)
    n, m, k = len(ids), len(sizes), 133
    plan = _plan_of_ids(ids)
    assert np.array_equal(np.diff(plan.offsets.cpu().numpy()[:m + 1]), np.asarray(sizes))
    x = torch.from_numpy(rng.standard_normal((n, k)).astype(np.float32)).to(DEV)
    w = torch.from_numpy((rng.standard_normal((C, k)) / np.sqrt(k)).astype(np.float32)).to(DEV)
    gamma = torch.from_numpy((1 + 0.1 * rng.standard_normal(C)).astype(np.float32)).to(DEV)
    beta = torch.from_numpy((0.1 * rng.standard_normal(C)).astype(np.float32)).to(DEV)
    pre, stats, y, pooled, argmax = _raw_fwd(x, w, gamma, beta, 1e-3, 2, plan)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(pre).all()) and bool(torch.isfinite(stats).all())
    assert float((y == 0).float().mean()) > 0.2          # ReLU zeros: ties inside the groups
    mx, first = _group_max_and_first_row(y.cpu(), ids, m)
    assert torch.equal(pooled.cpu(), mx)
    assert torch.equal(argmax.cpu().long(), first)
    counters = plan.scratch[(n, m, C)][:4 * m].view(torch.int32)
    assert int(counters.abs().sum()) == 0                # the tickets clean up behind themselves


# ------------------------------------------------------------------------------------------------------------------
# 2. exact product
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 3, 4, 84, 133, 146, 213, 256])
def test_product_is_exact_on_small_integers(k):
    """every partial sum is an integer below 2^24: pre == int64 product + gathered rows exactly (K tail, unaligned rows, gather)"""
    rng = np.random.default_rng(100 + k)
    sizes = _small_groups(200, rng)
    ids = _ids_of_sizes(sizes, rng)
    n, m = len(ids), len(sizes)
    plan = _plan_of_ids(ids)
    xi = rng.integers(-3, 4, size=(n, k))
    wi = rng.integers(-3, 4, size=(C, k))
    ai = rng.integers(-8, 9, size=(m, C))
    ones, zeros = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    x = torch.from_numpy(xi.astype(np.float32)).to(DEV)
    # the weight as a column slice of a wider matrix (row stride > K), as the second stage passes it
    wide = torch.full((C, k + 5), 1e30, device=DEV)
    wide[:, :k] = torch.from_numpy(wi.astype(np.float32)).to(DEV)
    add = torch.from_numpy(ai.astype(np.float32)).to(DEV)
    want = xi.astype(np.int64) @ wi.astype(np.int64).T
    pre = _raw_fwd(x, wide[:, :k], ones, zeros, 1e-3, 0, plan)[0]
    assert np.array_equal(pre.cpu().numpy().astype(np.int64), want) and bool((pre == pre.round()).all())
    pre = _raw_fwd(x, wide[:, :k].contiguous(), ones, zeros, 1e-3, 0, plan, add_rows=add)[0]
    assert np.array_equal(pre.cpu().numpy().astype(np.int64), want + ai[ids])


# ------------------------------------------------------------------------------------------------------------------
# 3. values and gradients against float64; 7. reproducibility
# ------------------------------------------------------------------------------------------------------------------
_VALUE_SIZES = [400, 130, 65, 64, 63]


def _value_inputs(k, split, seed):
    rng = np.random.default_rng(seed)
    sizes = np.concatenate([_VALUE_SIZES, rng.integers(1, 60, size=70)])
    ids = _ids_of_sizes(sizes, rng)
    n, m = len(ids), len(sizes)
    x = rng.standard_normal((n, k)).astype(np.float32)
    x[rng.random(n) < 0.5] *= 0.05     # rows whose variance behind the Linear is of the order of eps
    kw = k + C if split else k
    d = dict(ids=ids, n=n, m=m,
             x=torch.from_numpy(x), w=torch.from_numpy((rng.standard_normal((C, kw)) / np.sqrt(kw)).astype(np.float32)),
             gamma=torch.from_numpy((1 + 0.2 * rng.standard_normal(C)).astype(np.float32)),
             beta=torch.from_numpy((0.2 * rng.standard_normal(C)).astype(np.float32)),
             prev=torch.from_numpy((0.3 * rng.standard_normal((m, C))).astype(np.float32)) if split else None,
             gy=torch.from_numpy(rng.standard_normal((n, C)).astype(np.float32)),
             gp=torch.from_numpy(rng.standard_normal((m, C)).astype(np.float32)))
    return d


def _float64_stage(d, act, use_gy, use_gp):
    x, w, gamma, beta = (d[k].double().requires_grad_(True) for k in ('x', 'w', 'gamma', 'beta'))
    inv = torch.as_tensor(d['ids'])
    add = None
    if d['prev'] is not None:
        add = d['prev'].double() @ w[:, x.size(1):].t()
        add.retain_grad()
        pre = x @ w[:, :x.size(1)].t() + add[inv]
    else:
        pre = x @ w.t()
    z = torch.nn.functional.layer_norm(pre, (C,), gamma, beta, 1e-3)
    y = torch.nn.functional.gelu(z) if act == 'gelu' else torch.relu(z)
    pooled = torch.full((d['m'], C), float('-inf'), dtype=torch.float64).scatter_reduce(
        0, inv.view(-1, 1).expand(-1, C), y, reduce='amax')
    terms = ([(y * d['gy'].double()).sum()] if use_gy else []) + ([(pooled * d['gp'].double()).sum()] if use_gp else [])
    sum(terms).backward()
    out = dict(y=y.detach(), pooled=pooled.detach(), dx=x.grad, dw=w.grad, dgamma=gamma.grad, dbeta=beta.grad)
    if add is not None:
        out['dadd'] = add.grad
    return out


def _gpu_stage(d, act, fused, plan, use_gy, use_gp):
    """the stage through the fused node, or through today's modules (tall_linear -> add_layer_norm -> segment_reduce, with
    concat_gather in front of a second stage)"""
    from sst_amd import kernels as K
    from sst_amd.dense import add_layer_norm, tall_linear
    from sst_amd.sir_stage import sir_stage
    from sst_amd.voxel_encoder import DynamicVFELayerV2
    x = d['x'].to(DEV).requires_grad_(True)
    kw = d['w'].size(1)
    layer = DynamicVFELayerV2(kw, C, dict(type='LN', eps=1e-3), act=act).to(DEV)
    with torch.no_grad():
        layer.linear.weight.copy_(d['w'])
        layer.norm.weight.copy_(d['gamma'])
        layer.norm.bias.copy_(d['beta'])
    w = layer.linear.weight
    add = lin = None
    if fused:
        if d['prev'] is not None:
            add = tall_linear(d['prev'].to(DEV), w[:, x.size(1):])
            add.retain_grad()
            y, pooled = sir_stage(x, w[:, :x.size(1)], layer.norm, layer.act, plan, add_rows=add)
        else:
            y, pooled = sir_stage(x, w, layer.norm, layer.act, plan)
    else:
        xin = x
        if d['prev'] is not None:
            xin = K.concat_gather(x, d['prev'].to(DEV), plan.inverse, lambda part: K.segment_reduce(part, plan, 'sum'))
        lin = tall_linear(xin, w)                      # DynamicVFELayerV2.forward, with the Linear's output kept
        lin.retain_grad()
        y = add_layer_norm(lin, None, layer.norm, act=layer.act)
        pooled = K.segment_reduce(y, plan, 'max')
    # an upstream gradient that is not used is ABSENT from the backward (None), not a tensor of zeros
    terms = ([(y * d['gy'].to(DEV)).sum()] if use_gy else []) + ([(pooled * d['gp'].to(DEV)).sum()] if use_gp else [])
    sum(terms).backward()
    out = dict(y=y.detach(), pooled=pooled.detach(), dx=x.grad, dw=w.grad, dgamma=layer.norm.weight.grad,
               dbeta=layer.norm.bias.grad)
    if d['prev'] is not None:
        if fused:
            out['dadd'] = add.grad
        else:   # the rows the split form adds receive the group sums of the gradient at the Linear's output
            out['dadd'] = torch.zeros(d['m'], C, dtype=torch.float64).index_add_(0, torch.as_tensor(d['ids']),
                                                                                  lin.grad.cpu().double())
    return {k: v.detach().cpu().double() for k, v in out.items()}


def _check_against_float64(d, act, use_gy=True, use_gp=True):
    """the issue's bar, per quantity: fused error <= 2 x the composed path's error on the same inputs + 8 ulp of the largest
    reference magnitude, and inside the project's 1e-3 parity bar"""
    plan = _plan_of_ids(d['ids'])
    ref = _float64_stage(d, act, use_gy, use_gp)
    fused = _gpu_stage(d, act, True, plan, use_gy, use_gp)
    comp = _gpu_stage(d, act, False, plan, use_gy, use_gp)
    report = {}
    for key, want in ref.items():
        ef = float((fused[key] - want).abs().max())
        ec = float((comp[key] - want).abs().max())
        ulp = float(np.spacing(np.float32(want.abs().max())))
        report[key] = (ef, ec, ulp)
        print(f'sir_stage {act} k={d["x"].size(1)}{"+add" if d["prev"] is not None else ""} {key}: fused {ef:.3e} composed {ec:.3e} '
              f'ulp {ulp:.3e}')
    for key, (ef, ec, ulp) in report.items():
        assert ef <= 2 * ec + 8 * ulp, (key, ef, ec, ulp)
        assert ef < 1e-3, (key, ef)
    return fused


@pytest.mark.parametrize('act', ['gelu', 'relu'])
@pytest.mark.parametrize('k,split', [(84, False), (133, False), (213, False), (128, True)])
def test_values_and_gradients_against_float64(k, split, act):
    _check_against_float64(_value_inputs(k, split, seed=1000 + k), act)


@pytest.mark.parametrize('use_gy,use_gp', [(True, False), (False, True)])
def test_gradients_with_one_upstream_gradient_absent(use_gy, use_gp):
    _check_against_float64(_value_inputs(128, True, seed=77), 'gelu', use_gy, use_gp)


def test_two_runs_are_bit_identical():
    d = _value_inputs(213, False, seed=1213)
    plan = _plan_of_ids(d['ids'])
    from sst_amd.sir_stage import sir_stage
    norm = torch.nn.LayerNorm(C, eps=1e-3).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(d['gamma'])
        norm.bias.copy_(d['beta'])
    runs = []
    for _ in range(2):
        x = d['x'].to(DEV).requires_grad_(True)
        w = d['w'].to(DEV).requires_grad_(True)
        norm.weight.grad = norm.bias.grad = None
        y, pooled, (argmax, pre, stats) = sir_stage(x, w, norm, 'gelu', plan, return_saved=True)
        ((y * d['gy'].to(DEV)).sum() + (pooled * d['gp'].to(DEV)).sum()).backward()
        runs.append([t.detach().clone() for t in (y, pooled, argmax, pre, stats, x.grad, w.grad, norm.weight.grad, norm.bias.grad)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------
# 4. routing, exact
# ------------------------------------------------------------------------------------------------------------------
def test_pooling_gradient_is_routed_to_the_argmax_rows_exactly():
    """dy = 0, integer dpooled, integer data, gamma = 1, ReLU: the backward equals, bit for bit, sst_add_layernorm_act_bwd_f32 fed
    the gradient scattered explicitly to the arg-max rows (both run the same row arithmetic, csrc/ln_rows.h)"""
    from sst_amd import _lib
    from sst_amd.dense import add_ln_act_bwd
    rng = np.random.default_rng(5)
    sizes = np.concatenate([[200, 65, 64, 63], rng.integers(1, 12, size=60)])
    ids = _ids_of_sizes(sizes, rng)
    n, m, k = len(ids), len(sizes), 133
    plan = _plan_of_ids(ids)
    x = torch.from_numpy(rng.integers(-3, 4, size=(n, k)).astype(np.float32)).to(DEV)
    w = torch.from_numpy(rng.integers(-2, 3, size=(C, k)).astype(np.float32)).to(DEV)
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    pre, stats, y, pooled, argmax = _raw_fwd(x, w, gamma, beta, 1e-3, 2, plan)
    dpooled = torch.from_numpy(rng.integers(-4, 5, size=(m, C)).astype(np.float32)).to(DEV)
    lib = _lib.load()

    def fused_bwd(dy):
        d_pre = torch.full((n, C), float('nan'), device=DEV)
        dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        ws = torch.empty(int(lib.sst_sir_gather_segmax_bwd_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
        rc = lib.sst_sir_gather_segmax_bwd_f32(_lib.ptr(dy), _lib.ptr(dpooled), _lib.ptr(argmax), _lib.ptr(plan.inverse),
                                               _lib.ptr(pre), _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta), 2, n, C, m,
                                               _lib.ptr(d_pre), _lib.ptr(dg), _lib.ptr(db), _lib.ptr(ws), _lib.stream_ptr())
        assert rc == 0
        return d_pre, dg, db

    scattered = torch.zeros(n, C, device=DEV)
    scattered.scatter_(0, argmax.long(), dpooled)          # each dpooled[g, c] on row argmax[g, c] and nowhere else
    assert int((scattered != 0).sum()) == int((dpooled != 0).sum())
    want = add_ln_act_bwd(scattered, pre, stats, gamma, beta, 'relu')
    for dy in (None, torch.zeros(n, C, device=DEV)):
        got = fused_bwd(dy)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    assert bool((want[0] != 0).any())


# ------------------------------------------------------------------------------------------------------------------
# 5. the reference's golden through the switch
# ------------------------------------------------------------------------------------------------------------------
def _spy_on_sir_stage(monkeypatch):
    from sst_amd import voxel_encoder
    calls = []
    real = voxel_encoder.sir_stage

    def spy(*args, **kwargs):
        calls.append((tuple(args[0].shape), kwargs.get('add_rows') is not None))
        return real(*args, **kwargs)
    monkeypatch.setattr(voxel_encoder, 'sir_stage', spy)
    return calls


def test_fused_sir_matches_reference_golden(monkeypatch):
    import sst_amd
    g = load_golden('sir.npz')
    sir = sst_amd.build_backbone(dict(type='SIR', num_blocks=3, in_channels=[84, 133, 133],
                                      feat_channels=[[128, 128]] * 3, rel_mlp_hidden_dims=[[16, 32]] * 3,
                                      norm_cfg=dict(type='LN', eps=1e-3), mode='max', xyz_normalizer=[20, 20, 4],
                                      act='gelu', unique_once=True))
    sd = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith('w::')}
    sir.load_state_dict(sd, strict=True)
    sir.to(DEV).train()
    sst_amd.enable_fused_sir(sir)
    calls = _spy_on_sir_stage(monkeypatch)
    feats = torch.from_numpy(g['in::features']).to(DEV).requires_grad_(True)
    pts_feats, cluster_feats, cluster_coors = sir(torch.from_numpy(g['in::points']).to(DEV), feats,
                                                  torch.from_numpy(g['in::coors']).to(DEV),
                                                  torch.from_numpy(g['in::f_cluster']).to(DEV))
    assert [(c[0][1], c[1]) for c in calls] == [(84, False), (128, True), (133, False), (128, True), (133, False), (128, True)]
    np.testing.assert_array_equal(cluster_coors.cpu().numpy(), g['out::cluster_coors'])
    np.testing.assert_allclose(pts_feats.detach().cpu().numpy(), g['out::pts_feats'], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(cluster_feats.detach().cpu().numpy(), g['out::cluster_feats'], rtol=1e-3, atol=1e-3)
    ((pts_feats * torch.from_numpy(g['in::g_pts']).to(DEV)).sum()
     + (cluster_feats * torch.from_numpy(g['in::g_cluster']).to(DEV)).sum()).backward()
    np.testing.assert_allclose(feats.grad.cpu().numpy(), g['out::grad_features'], rtol=2e-3, atol=2e-3)
    for name, p in sir.named_parameters():
        assert p.grad is None or bool(torch.isfinite(p.grad).all()), name
    assert sir.block_list[0].vfe_layers[1].linear.weight.grad.abs().sum() > 0


# ------------------------------------------------------------------------------------------------------------------
# 6. fall-backs
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['width32', 'batchnorm', 'foreign_inverse'])
def test_ineligible_layers_take_the_composed_path_unchanged(kind, monkeypatch):
    import sst_amd
    g = torch.Generator().manual_seed(21)
    n = 3000
    coors = torch.stack([torch.randint(0, 2, (n,), generator=g), torch.randint(0, 60, (n,), generator=g)], 1).to(DEV)
    feats = torch.randn(n, 16, generator=g).to(DEV)
    width = 32 if kind == 'width32' else 128
    norm_cfg = dict(type='naiveSyncBN1d', eps=1e-3, momentum=0.01) if kind == 'batchnorm' else dict(type='LN', eps=1e-3)
    torch.manual_seed(3)
    layer = sst_amd.SIRLayer(in_channels=16, feat_channels=[width, width], rel_mlp_hidden_dims=[16], norm_cfg=norm_cfg,
                             mode='max', act='gelu', return_point_feats=True).to(DEV).eval()
    extra = {}
    if kind == 'foreign_inverse':
        uniq, inv = torch.unique(coors, dim=0, return_inverse=True)
        extra = dict(unq_inv_once=inv, new_coors_once=uniq)
    calls = _spy_on_sir_stage(monkeypatch)

    def run(flag):
        sst_amd.enable_fused_sir(layer, flag)
        if 'unq_inv_once' in extra:
            extra['unq_inv_once'] = extra['unq_inv_once'].clone()     # a fresh tensor: no plan attached by an earlier run
        x = feats.clone().requires_grad_(True)
        pf, gf = layer(x, coors, **extra)
        (pf.sum() + (gf * gf).sum()).backward()
        return pf.detach(), gf.detach(), x.grad

    off, on = run(False), run(True)
    assert calls == []
    for a, b in zip(off, on):
        assert torch.equal(a, b)
    if kind == 'foreign_inverse':     # the same layer does fuse on a grouping of this library's own
        extra.clear()
        fused = run(True)
        assert len(calls) == 2
        assert float((fused[0] - off[0]).abs().max()) < 1e-3
