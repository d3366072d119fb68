"""CPU: the float64 models and operand recipes of tests/bf16_exact_ref.py checked on their own - the rounding step against a
bit-manipulation RNE at every bf16 neighbour pair's midpoint, the models with their rounding steps switched off against plain
torch float64 autograd of the same chain, and every recipe against its exactness condition at every size the GPU tests use."""
import pytest
import torch

import bf16_exact_ref as R

TAIL_BF16_COUNTS = 272      # tests/test_gpu_tail_exact.py: 1 .. 272 (128 tokens per workgroup)
TAIL_F32_COUNTS = 144       # ... 1 .. 2 * 64 + 16 (64 tokens per workgroup of csrc/layer_tail_x6.hip)
SMALL = 49                  # tests/test_gpu_bf16_linear_exact.py: 1 .. 49
LN_LARGE = 4099             # ... and one count that is no multiple of a kernel's row tile


def test_rne_is_round_to_nearest_even_at_every_midpoint():
    """all 2^16 bf16 bit patterns b (finite): the fp32 values b.7fff, b.8000 (the tie) and b.8001 between b and its upper
    neighbour, and b itself"""
    b = torch.arange(0, 1 << 16, dtype=torch.int64)
    b = b[((b >> 7) & 0xff) != 0xff]                                      # no inf / nan
    for low in (0x0000, 0x7fff, 0x8000, 0x8001, 0xffff):
        u = (b << 16) | low
        ok = ((u >> 23) & 0xff) != 0xff
        u = u[ok]
        f = (u - ((u >> 31) << 32)).to(torch.int32).view(torch.float32)   # the bit pattern as a signed 32-bit integer
        want = R.rne_bits(u)
        finite = ((want >> 7) & 0xff) != 0xff                             # a value that rounds up to inf stays out
        got = R.rne(f.double()).float().view(torch.int32).to(torch.int64)
        got = (got >> 16) & 0xffff
        assert torch.equal(got[finite], want[finite]), hex(low)
    # ties go to the even neighbour, in both directions
    one = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=torch.float64)
    assert R.rne(one).tolist() == [1.0, 1.0 + 2.0 ** -6]


def _params64(seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc)   # noqa: E731
    return dict(w_out=r(128, 128, sc=0.09), b_out=r(128, sc=0.1), w1=r(256, 128, sc=0.09), b1=r(256, sc=0.1),
                w2=r(128, 256, sc=0.06), b2=r(128, sc=0.1), n1w=1 + r(128, sc=0.2), n1b=r(128, sc=0.1),
                n2w=1 + r(128, sc=0.2), n2b=r(128, sc=0.1))


@pytest.mark.parametrize('act,with_pos', [('gelu', True), ('relu', False)])
def test_models_without_rounding_are_the_float64_chain(act, with_pos):
    """tail_fwd / tail_bwd with bf16=False against torch autograd (`_ref64` of tests/test_gpu_encoder_tail.py): the model is the
    operation, not a copy of a kernel"""
    from test_gpu_encoder_tail import _ref64
    m, eps = 37, 1e-5
    g = torch.Generator().manual_seed(1)
    o, x = torch.randn(m, 128, generator=g), torch.randn(m, 128, generator=g)
    p = _params64(2)
    pos = (torch.randn(144, 128, generator=g), torch.randint(0, 144, (m,), generator=g, dtype=torch.int32)) if with_pos else None
    ref = _ref64(o, x, p, act, eps, pos)
    pd = {k: v.double() for k, v in p.items()}
    rows = pos[0].double()[pos[1].long()] if with_pos else None
    mod = R.tail_fwd(o.double(), x.double(), pd, act, eps, rows, bf16=False)
    close = lambda a, b: float((a - b.detach()).abs().max()) <= 1e-12 * max(1.0, float(b.detach().abs().max()))   # noqa: E731
    for k in ('s1', 'y1', 'pre', 'h', 's2', 'y2') + (('y2p',) if with_pos else ()):
        assert close(mod[k], ref[k]), k
    dy2 = torch.randn(m, 128, generator=g).double()
    dy2p = torch.randn(m, 128, generator=g).double() if with_pos else None
    loss = (ref['y2'] * dy2).sum() + ((ref['y2p'] * dy2p).sum() if with_pos else 0)
    grads = torch.autograd.grad(loss, [ref['s2'], ref['pre'], ref['s1'], ref['o'], ref['params']['n2w'], ref['params']['n2b'],
                                       ref['params']['n1w'], ref['params']['n1b']])
    st = lambda a, b: torch.stack([a, b], 1)   # noqa: E731
    bw = R.tail_bwd(dy2, dy2p, mod['s2'], st(mod['mean2'], mod['rstd2']), mod['pre'], mod['s1'], st(mod['mean1'], mod['rstd1']),
                    pd, act, bf16=False)
    for got, want in zip((bw['ds2'], bw['dpre'], bw['ds1'], bw['d_o'], bw['dn2w_rows'].sum(0), bw['dn2b_rows'].sum(0),
                          bw['dn1w_rows'].sum(0), bw['dn1b_rows'].sum(0)), grads):
        assert close(got, want)


def test_linear_and_layernorm_models_without_rounding_are_float64():
    g = torch.Generator().manual_seed(3)
    x, w, b, aux = (torch.randn(s, generator=g).double() for s in ((9, 128), (256, 128), (256,), (9, 256)))
    acc = x @ w.t() + b
    a = aux.clone().requires_grad_(True)
    torch.nn.functional.gelu(a).sum().backward()
    for epi, want in ((R.EPI_BIAS, acc), (R.EPI_GELU, torch.nn.functional.gelu(acc)), (R.EPI_RELU, torch.relu(acc)),
                      (R.EPI_MUL_GELU_GRAD, acc * a.grad), (R.EPI_MUL_RELU_GRAD, acc * (aux > 0)), (R.EPI_ADD, acc + aux)):
        assert float((R.linear(x, w, b, epi, aux, bf16=False)['y'] - want).abs().max()) < 1e-12, epi
    s = torch.randn(9, 128, generator=g).double().requires_grad_(True)
    lw, lb, dy = (torch.randn(sh, generator=g).double() for sh in ((128,), (128,), (9, 128)))
    lw.requires_grad_(True), lb.requires_grad_(True)
    y = torch.nn.functional.layer_norm(s, (128,), lw, lb, 1e-5)
    f = R.ln_fwd(s.detach(), lw.detach(), lb.detach(), 1e-5, bf16=False)
    assert float((f['y'] - y.detach()).abs().max()) < 1e-12
    gs, gw, gb = torch.autograd.grad((y * dy).sum(), [s, lw, lb])
    bw = R.ln_bwd(dy, s.detach(), f['mean'], f['rstd'], lw.detach(), bf16=False)
    assert float((bw['dx'] - gs).abs().max()) < 1e-12 and float((bw['dw_rows'].sum(0) - gw).abs().max()) < 1e-12 \
        and float((bw['db_rows'].sum(0) - gb).abs().max()) < 1e-12


@pytest.mark.parametrize('k,n', [(128, 128), (128, 256), (256, 128)])
def test_recipe_i_linear_is_exact(k, n):
    """at the small counts, at 4096 rows of the large ones (a row's exactness does not depend on the others), and by the bound
    256 * 8 * 4 + 8 + 8 < 2^24 at any count; results above 256 occur, so the store rounds"""
    for m in (SMALL, 4096):
        r = R.recipe_i_linear(m, k, n)
        for epi in (R.EPI_BIAS, R.EPI_RELU, R.EPI_MUL_RELU_GRAD, R.EPI_ADD):
            tr = R.Trace()
            out = R.linear(r['x'], r['w'], r['bias'], epi, r['aux'], tr=tr)
            assert R.assert_exact(tr) > 8
        assert float(out['acc'].abs().max()) > 256 and not torch.equal(out['y'], out['v'])
    assert 256 * 8 * 4 + 8 + 8 < 2 ** 24
    tr = R.Trace()
    R.ln_fwd(out['acc'][:, :128] + r['aux'][:, :128], torch.ones(128).double(), torch.zeros(128).double(), 1e-5, tr=tr)
    assert R.assert_exact(tr, only=('ln.mean',)) > 8


@pytest.mark.parametrize('k,n', [(128, 128), (128, 256), (256, 128)])
def test_recipe_f_linear_is_exact_and_shows_where_the_activation_is_taken(k, n):
    r = R.recipe_f_linear(SMALL, k, n)
    for epi in (R.EPI_BIAS, R.EPI_GELU, R.EPI_RELU, R.EPI_MUL_RELU_GRAD, R.EPI_ADD):
        tr = R.Trace()
        out = R.linear(r['x'], r['w'], r['bias'], epi, r['aux'], tr=tr)
        assert R.assert_exact(tr) > 8
    out = R.linear(r['x'], r['w'], r['bias'], R.EPI_GELU)
    assert not torch.equal(out['pre'], out['acc'])                        # the stored pre-activation is rounded
    wrong = R.rne(R.gelu64(out['acc']))                                   # GELU at the unrounded pre-activation, then stored
    share = float(R.within_bf16(wrong, out['v'], R.gelu_slack(out['pre'], out['v'])).double().mean())
    assert share > 0.01, share                                            # ... breaks the rule at more than 1 % of the elements
    assert not bool(R.within_bf16(out['y'], out['v'], R.gelu_slack(out['pre'], out['v'])).any())


@pytest.mark.parametrize('k,n', [(128, 128), (128, 256), (256, 128)])
def test_recipe_s_linear_is_exact_for_gaussian_inputs(k, n):
    r = R.recipe_s_linear(SMALL, k, n)
    assert int((r['w'] != 0).sum(1).max()) == (2 if n < k else 1)
    if n >= k:                                      # one scaled input per output: exact for any input
        tr = R.Trace()
        R.linear(r['x'], r['w'], None, R.EPI_RELU, tr=tr)
        R.assert_exact(tr)


@pytest.mark.parametrize('m', [SMALL, LN_LARGE])
def test_recipe_b_layernorm_backward_is_exact(m):
    r = R.recipe_b_ln(m)
    tr = R.Trace()
    out = R.ln_bwd(r['dy'] + r['dy2'], r['s'], r['st'][:, 0], r['st'][:, 1], r['w'], tr=tr)
    assert R.assert_exact(tr) >= 2
    assert torch.equal(r['s'].to(R.BF).double(), r['s']) and not torch.equal(out['dx'], out['dxv'])   # bf16 operands; the store rounds
    assert set(r['st'][:, 1].tolist()) == {1.0, 0.5, 0.25}


@pytest.mark.parametrize('bf16,m', [(True, TAIL_BF16_COUNTS), (False, TAIL_F32_COUNTS)])
def test_recipe_b_tail_backward_is_exact(bf16, m):
    """every stage of the ReLU backward of either tail at the largest count (column sums grow with m; everything else is per row)"""
    t, p = R.recipe_b_tail(m)
    for dy2p in (t['dy2p'], None):
        tr = R.Trace()
        out = R.tail_bwd(t['dy2'], dy2p, t['s2'], t['st2'], t['pre'], t['s1'], t['st1'], p, 'relu', bf16=bf16, tr=tr)
        assert R.assert_exact(tr) >= 2
    for k in ('dy2', 'dy2p', 's2', 's1', 'pre'):
        assert torch.equal(t[k].to(R.BF).double(), t[k]), k
    assert bool((t['pre'] == 0).any()) and bool((t['pre'] > 0).any()) and bool((t['pre'] < 0).any())
    assert float(out['ds1'].abs().max()) > 0 and float(out['d_o'].abs().max()) > 0
    # GELU: exactness is claimed up to ds2 (and norm2's parameter gradients) only
    tr = R.Trace()
    R.tail_bwd(t['dy2'], t['dy2p'], t['s2'], t['st2'], t['pre'], t['s1'], t['st1'], p, 'gelu', bf16=bf16, tr=tr)
    R.assert_exact(tr, only=('ds2.',))


@pytest.mark.parametrize('bf16,m', [(True, TAIL_BF16_COUNTS), (False, TAIL_F32_COUNTS)])
def test_tail_forward_recipes_are_exact_where_claimed(bf16, m):
    eps = 1e-5
    o, x = R.tail_inputs_i(m)
    tr = R.Trace()
    R.tail_fwd(o, x, R.tail_params_i(), 'relu', eps, bf16=bf16, tr=tr)
    assert R.assert_exact(tr, only=('s1.',)) > 8                      # recipe I: s1 and its mean
    o, x = R.tail_inputs_s(m)
    p = R.tail_params_s()
    tr = R.Trace()
    y1 = None if bf16 else R.tail_fwd(o, x, p, 'relu', eps, bf16=False)['y1'].float().double()   # an fp32 y1, as a kernel stores it
    out = R.tail_fwd(o, x, p, 'relu', eps, bf16=bf16, tr=tr, y1=y1)
    # recipe S: pre and h from any y1; in the bf16 mode s2 as well (y1 a multiple of 2^-5 by the choice of norm1's parameters)
    assert R.assert_exact(tr, only=('pre.',) + (('s2.',) if bf16 else ())) > 2
    if bf16:
        assert float(out['y1'].abs().min()) >= 4 and bool((out['h'] == 0).any()) and bool((out['h'] > 0).any())
