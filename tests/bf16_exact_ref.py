"""float64 models of the dense kernels of the reduced-precision mode (csrc/dense_bf16.hip, the bf16 LayerNorm kernels of
csrc/dense.hip, csrc/layer_tail_bf16.hip) and of the exact-split encoder tail (csrc/layer_tail_x6.hip), the operand recipes under
which a correct kernel must return the model BIT FOR BIT, and the proof obligation (`assert_exact`) that goes in front of every
such comparison.  No GPU, no kernel code: plain torch in float64 on the CPU.

Rounding points.  The kernels accumulate in fp32 and store bf16 with one round-to-nearest-even conversion (`pack2` =
v_cvt_pk_bf16_f32).  `rne` below is that conversion and the ONLY rounding the models contain; it stands exactly where a kernel
stores a bf16 value or reads one back (models called with bf16=False - the fp32 tail - contain none):
  linear      acc = x W^T + b (fp32); GELU / ReLU: pre = rne(acc) is stored and the activation acts on the ROUNDED pre;
              x GELU' / x ReLU' / add: the aux operand is applied to the unrounded acc; y = rne(...)
  LayerNorm   the statistics and y are formed from the UNROUNDED fp32 sum; stored: s = rne(sum), y = rne(y), y + pos = rne(y + p)
              (p added to the unrounded y)
  LN backward d = dy (+ dy2) (fp32), xhat = (s - mean) rstd from the STORED s and statistics; dx = rne(...); d(gamma), d(beta) fp32
  tail        bf16: s1, y1, pre, h, s2, y2, y2p, ds2, dpre, ds1, d_o are rounded where they are stored, and what is stored is what
              the next product reads; d(y1) = ds2 + dpre W1 stays fp32.  fp32: nothing is rounded.  The activation acts on the
              stored pre-activation, as in the linears.

Exactness.  A stage is bit-exact when every intermediate of the model IS an fp32 number and every sum's partial sums are fp32
numbers in any order: all terms are multiples of a granule 2^-q and the sum of their absolute values is below 2^24 granules.
The models record both kinds of facts in a `Trace`; `assert_exact(trace)` checks them on the actual operands before anything is
launched.  Where no such argument exists (GELU, the LayerNorm outputs, rstd) the comparison is element by element against the
model fed with the kernel's own stored input: `within_bf16` / `within_f32` with a slack derived where it is used.

Recipes (all values are bf16 numbers unless said otherwise):
  I  integers: x, aux, residual in [-8, 8], weights in [-4, 4], biases in [-8, 8].  K <= 256: sum |terms| <= 256 * 32 + 16 < 2^24.
     Results above 256 are NOT bf16 numbers: the store really rounds.
  F  recipe I with the weights / 64, biases / 8 and aux / 4: equally exact, pre-activations of magnitude <= 10 with up to 10
     significant bits - where rounding the pre-activation changes GELU by more than the elementwise rule allows.
  S  selection weights: one entry +-2^e (e in [-2, 2]) per weight row, every input column used; zero biases.  A product is one
     exactly scaled input: bit-exact for arbitrary inputs.  Two entries per row for K = 256 -> N = 128 (every column used once).
  B  crafted statistics for the backward kernels: mean integer in [-8, 8] and rstd in {1, 1/2, 1/4} per row, the saved sum
     s = mean + delta / rstd with delta integer in [-2, 2] (so xhat = delta, s integer in [-16, 16]), dy in [-2, 2], dy2 in [-1, 1],
     LayerNorm weights in [-2, 2] (norm2) and {-1, 0, 1} (norm1), pre-activations in [-3, 3] (ReLU), W2 with two entries of
     {+-1, +-2} per hidden column, W1 with three entries +-1 per model column, W_o a selection matrix (one +-2^e per input
     column): ds2 has granule 2^-9, d(y1) granule 2^-9 and |d(y1)| of a few tens, ds1 granule 2^-18; `assert_exact` holds with
     two bits to spare at every token count the tests use (tests/test_bf16_exact_host.py).
"""
import math

import torch

BF = torch.bfloat16
EPI_BIAS, EPI_GELU, EPI_RELU, EPI_MUL_GELU_GRAD, EPI_MUL_RELU_GRAD, EPI_ADD = range(6)


def rne(t, on=True):
    """fp32 -> bf16 round-to-nearest-even of a float64 tensor that holds fp32 numbers (asserted wherever bit-exactness is
    claimed: `.float()` is then the identity); off: the identity (fp32 storage)"""
    return t.float().to(BF).double() if on else t


def rne_bits(u):
    """the same conversion by bit manipulation on the int64 tensor of fp32 bit patterns (finite values) -> bf16 bit patterns"""
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


# ------------------------------------------------------------------------------------------------------------------
# the proof obligation
# ------------------------------------------------------------------------------------------------------------------
def granule(t, dim=None):
    """the largest power of two that divides every entry of t (per row with dim=1, as a column); 2^60 for all-zero input"""
    a = t.double().abs()
    mant, exp = torch.frexp(a)                                  # a = mant * 2^exp, mant in [0.5, 1)
    mi = (mant * 2.0 ** 53).to(torch.int64)
    low = (mi & -mi).double()                                   # lowest set bit of the 53-bit significand
    g = torch.where(a > 0, low * torch.exp2((exp - 53).double()), torch.full_like(a, 2.0 ** 60))
    return g.min() if dim is None else g.min(dim, keepdim=True).values


class Trace:
    """what a model run claims: values that must be fp32 numbers, sums whose absolute terms must stay below 2^24 granules"""

    def __init__(self):
        self.values, self.sums = [], []

    def value(self, name, t):
        self.values.append((name, t))
        return t

    def sum(self, name, abs_sum, gran):
        self.sums.append((name, abs_sum, gran))


def _val(tr, name, t):
    return tr.value(name, t) if tr is not None else t


def assert_exact(tr, only=None):
    """every recorded value equals its own cast to float32; every recorded sum of absolute terms < 2^24 granules.
    `only`: stage-name prefixes to check (the stages a test claims bit-exact).  -> the smallest margin in bits"""
    ok = lambda n: only is None or any(n.startswith(p) for p in only)   # noqa: E731
    checked, margin = 0, 60.0
    for name, t in tr.values:
        if ok(name):
            assert torch.equal(t.float().double(), t), f'{name}: not an fp32 number'
            checked += 1
    for name, abs_sum, gran in tr.sums:
        if ok(name):
            ratio = float((abs_sum / gran).max()) if abs_sum.numel() else 0.0
            assert ratio < 2.0 ** 24, f'{name}: sum of absolute terms is 2^{math.log2(max(ratio, 1)):.1f} granules'
            margin = min(margin, 24.0 - math.log2(max(ratio, 1.0)))
            checked += 1
    assert checked > 0, 'nothing was claimed'
    return margin


def _matmul(x, w, tr, name):
    """x W^T in float64; records that every partial sum is an fp32 number"""
    if tr is not None:
        nnz = int((w != 0).sum(1).max())
        if nnz <= 4:      # sparse rows: the terms of every output element on their own (one term: nothing is summed)
            idx = (w != 0).double().topk(nnz, dim=1).indices                       # [n, nnz]
            terms = x[:, idx] * w.gather(1, idx)                                   # [m, n, nnz]
            if nnz > 1:
                tr.sum(name, terms.abs().sum(-1), granule(terms, -1)[..., 0])
        else:
            tr.sum(name, x.abs() @ w.abs().t(), granule(x, 1) * granule(w))
    return x @ w.t()


# ------------------------------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------------------------------
def linear(x, w, bias, epi, aux=None, bf16=True, tr=None, name='linear'):
    """sst_tall_linear_bf16 -> dict(y, pre (GELU / ReLU), acc (unrounded x W^T + b))"""
    acc = _matmul(x, w, tr, name + '.acc')
    if bias is not None:
        if tr is not None:
            tr.sum(name + '.bias', x.abs() @ w.abs().t() + bias.abs(), torch.minimum(granule(x, 1) * granule(w), granule(bias)))
        acc = acc + bias
    _val(tr, name + '.acc', acc)
    out = dict(acc=acc)
    if epi in (EPI_GELU, EPI_RELU):
        pre = rne(acc, bf16)
        out['pre'] = pre
        v = gelu64(pre) if epi == EPI_GELU else torch.relu(pre)
    elif epi == EPI_MUL_GELU_GRAD:
        v = acc * gelu_grad64(aux)
    elif epi == EPI_MUL_RELU_GRAD:
        v = acc * (aux > 0).double()
    elif epi == EPI_ADD:
        v = _val(tr, name + '.add', acc + aux)
        if tr is not None:
            tr.sum(name + '.add', acc.abs() + aux.abs(), torch.minimum(granule(acc, 1), granule(aux, 1)))
    else:
        v = acc
    out['y'] = rne(v, bf16)
    out['v'] = v
    return out


def ln_fwd(ssum, w, b, eps, pos_rows=None, bf16=True, tr=None, name='ln'):
    """LayerNorm of the UNROUNDED sum -> dict(s, mean, rstd, y, yp, xhat)"""
    if tr is not None:
        tr.sum(name + '.mean', ssum.abs().sum(1, keepdim=True), granule(ssum, 1))
    mean = _val(tr, name + '.mean', ssum.mean(1, keepdim=True))
    c = ssum - mean
    rstd = 1.0 / torch.sqrt((c * c).mean(1, keepdim=True) + eps)
    yv = c * rstd * w + b
    out = dict(s=rne(ssum, bf16), mean=mean[:, 0], rstd=rstd[:, 0], y=rne(yv, bf16), yv=yv, xhat=c * rstd, yp=None, ypv=None)
    if pos_rows is not None:
        out['ypv'] = yv + pos_rows
        out['yp'] = rne(out['ypv'], bf16)
    return out


def ln_bwd(d, s, mean, rstd, w, bf16=True, tr=None, name='lnb'):
    """LayerNorm backward from the stored sum and statistics: d = upstream gradient (dy + dy2, fp32) -> dict(dx, dxv, dw_rows,
    db_rows): dw_rows / db_rows are the per-token terms of d(gamma) / d(beta) (their prefix sums are the results at every m)"""
    mean, rstd = mean[:, None], rstd[:, None]
    xhat = _val(tr, name + '.xhat', (_val(tr, name + '.c', s - mean)) * rstd)
    g = _val(tr, name + '.g', d * w)
    if tr is not None:
        tr.sum(name + '.sg', g.abs().sum(1, keepdim=True), granule(g, 1))
        tr.sum(name + '.sgx', (g * xhat).abs().sum(1, keepdim=True), granule(g, 1) * granule(xhat, 1))
    gx = _val(tr, name + '.gx', g * xhat)
    mg = _val(tr, name + '.mg', g.mean(1, keepdim=True))
    mgx = _val(tr, name + '.mgx', gx.mean(1, keepdim=True))
    t1 = _val(tr, name + '.g-mg', g - mg)
    t2 = _val(tr, name + '.xhat*mgx', xhat * mgx)
    dxv = _val(tr, name + '.dx', rstd * _val(tr, name + '.diff', t1 - t2))
    dw_rows = _val(tr, name + '.d*xhat', d * xhat)
    if tr is not None:
        tr.sum(name + '.dw', dw_rows.abs().sum(0), granule(dw_rows))
        tr.sum(name + '.db', d.abs().sum(0), granule(d))
    return dict(dx=rne(dxv, bf16), dxv=dxv, dw_rows=dw_rows, db_rows=d)


def tail_fwd(o, x, p, act, eps, pos_rows=None, bf16=True, tr=None, y1=None, pre=None, h=None):
    """the encoder tail, forward.  y1 / pre / h given: the stage behind them is fed with these (the kernel's own stored tensors)
    instead of the model's.  p: dict of float64 parameters (w_out, b_out, w1, b1, w2, b2, n1w, n1b, n2w, n2b)"""
    s1v = _matmul(o, p['w_out'], tr, 's1.acc') + p['b_out'] + x
    if tr is not None:
        tr.sum('s1.sum', o.abs() @ p['w_out'].abs().t() + p['b_out'].abs() + x.abs(),
               torch.minimum(torch.minimum(granule(o, 1) * granule(p['w_out']), granule(x, 1)), granule(p['b_out'])))
        tr.value('s1.v', s1v)
    l1 = ln_fwd(s1v, p['n1w'], p['n1b'], eps, None, bf16, tr, 's1.ln')
    y1_in = l1['y'] if y1 is None else y1
    prev = _matmul(y1_in, p['w1'], tr, 'pre.acc') + p['b1']
    _val(tr, 'pre.v', prev)
    pre_m = rne(prev, bf16)
    pre_in = pre_m if pre is None else pre
    hv = gelu64(pre_in) if act == 'gelu' else torch.relu(pre_in)
    h_m = rne(hv, bf16)
    h_in = h_m if h is None else h
    acc2 = _matmul(h_in, p['w2'], tr, 's2.acc')
    s2v = acc2 + p['b2'] + y1_in
    if tr is not None:
        tr.sum('s2.sum', h_in.abs() @ p['w2'].abs().t() + p['b2'].abs() + y1_in.abs(),
               torch.minimum(torch.minimum(granule(h_in, 1) * granule(p['w2']), granule(y1_in, 1)), granule(p['b2'])))
        tr.value('s2.v', s2v)
    l2 = ln_fwd(s2v, p['n2w'], p['n2b'], eps, pos_rows, bf16, None, 's2.ln')
    s2_abs = h_in.abs() @ p['w2'].abs().t() + p['b2'].abs() + y1_in.abs()
    return dict(s1=l1['s'], s1v=s1v, mean1=l1['mean'], rstd1=l1['rstd'], y1=l1['y'], y1v=l1['yv'], xhat1=l1['xhat'],
                pre=pre_m, prev=prev, h=h_m, hv=hv, s2=l2['s'], s2v=s2v, s2_abs=s2_abs, mean2=l2['mean'], rstd2=l2['rstd'],
                y2=l2['y'], y2v=l2['yv'], xhat2=l2['xhat'], y2p=l2['yp'], y2pv=l2['ypv'])


def tail_bwd(dy2, dy2p, s2, st2, pre, s1, st1, p, act, bf16=True, tr=None):
    """the encoder tail, backward, from the saved tensors and statistics (st = [m, 2] = mean | rstd)"""
    d = dy2 if dy2p is None else _val(tr, 'ds2.d', dy2 + dy2p)
    b2 = ln_bwd(d, s2, st2[:, 0], st2[:, 1], p['n2w'], bf16, tr, 'ds2.ln')
    ds2 = b2['dx']
    a1 = _val(tr, 'dpre.acc', _matmul(ds2, p['w2'].t(), tr, 'dpre.acc'))
    dprev = a1 * (gelu_grad64(pre) if act == 'gelu' else (pre > 0).double())
    dpre = rne(dprev, bf16)
    acc = _val(tr, 'ds1.acc', _matmul(dpre, p['w1'].t(), tr, 'ds1.acc'))
    dy1 = _val(tr, 'ds1.dy1', acc + ds2)
    if tr is not None:
        tr.sum('ds1.dy1', dpre.abs() @ p['w1'].abs() + ds2.abs(), torch.minimum(granule(dpre, 1) * granule(p['w1']), granule(ds2, 1)))
    b1 = ln_bwd(dy1, s1, st1[:, 0], st1[:, 1], p['n1w'], bf16, tr, 'ds1.ln')
    ds1 = b1['dx']
    d_ov = _val(tr, 'd_o.acc', _matmul(ds1, p['w_out'].t(), tr, 'd_o.acc'))
    return dict(ds2=ds2, dpre=dpre, dprev=dprev, a1=a1, dy1=dy1, ds1=ds1, d_o=rne(d_ov, bf16),
                dn2w_rows=b2['dw_rows'], dn2b_rows=b2['db_rows'], dn1w_rows=b1['dw_rows'], dn1b_rows=b1['db_rows'])


# ------------------------------------------------------------------------------------------------------------------
# the elementwise rule
# ------------------------------------------------------------------------------------------------------------------
ERF_ABS = 4e-7
"""|erf_as - erf|: 1.5e-7 of Abramowitz & Stegun 7.1.26 as the kernels state it, + the hardware reciprocal (1 ulp of t <= 1: 1.2e-7
through the polynomial's slope <= 1), + v_exp_f32 on -z^2 log2(e) (argument rounding z^2 * 1.44 * 2^-23 times e^(-z^2) <= 6.3e-8),
+ five fp32 roundings of the Horner chain and the final fma (6 * 2^-24 = 3.6e-8 at |values| <= 1.5): 3.7e-7, taken as 4e-7"""
RSTD_REL = 65 * 2.0 ** -24 + 2.0 ** -22
"""relative error of rstd: the 128 non-negative squares summed in fp32 (any order) are within 128 * 2^-24 of their sum, + one
rounding for `/ 128 + eps`; the inverse root halves that (64.5 * 2^-24), + the rsqrt instruction's 1 ulp and the rounding of the
centred values feeding the squares (2^-22 in all)"""


def gelu_slack(x, y):
    """|gelu_f(x) - gelu(x)| for an fp32 x: 0.5 |x| ERF_ABS + three fp32 roundings of the result"""
    return 0.5 * x.abs() * ERF_ABS + 3 * 2.0 ** -24 * y.abs()


def gelu_grad_slack(x):
    """|gelu_grad_f(x) - gelu'(x)|: 0.5 ERF_ABS for Phi, |x| 0.399 * (6.3e-8 + 2^-23) for x phi(x) with the hardware exponential,
    + three fp32 roundings at |gelu'| <= 1.13"""
    return 0.5 * ERF_ABS + x.abs() * 0.4 * 1.9e-7 + 3 * 2.0 ** -24 * 1.13


def ln_y_slack(xhat, w, yv, in_err=0.0):
    """|y - model| before the store: xhat carries RSTD_REL and two roundings (centre, scale), the product with gamma and the sum
    with beta (or their fma) two more (2^-22 in all on xhat w, 2^-24 on y); `in_err`: what an inexact INPUT adds (ln_in_err)"""
    return (xhat * w).abs() * (RSTD_REL + 2.0 ** -22) + 2.0 ** -24 * yv.abs() + in_err


def ln_in_err(delta, rstd, w, xhat):
    """what an error of at most `delta` (column [m, 1]) in every element of a LayerNorm's input moves y by: a centred value moves
    by <= 2 delta, the variance by <= 2 (2 delta) std, so rstd by <= 2 delta rstd relative: 2 delta rstd |w| (1 + |xhat|)"""
    return 2.0 * delta * rstd[:, None] * w.abs() * (1.0 + xhat.abs())


def within_bf16(got, model, slack):
    """element by element: |got - model| <= half a bf16 step of |model| (+ slack, which may move it into the next binade) + slack
    -> boolean tensor of violations"""
    got = got.double()
    mag = (model.abs() + slack).clamp_min(2.0 ** -126)
    half = torch.exp2(torch.floor(torch.log2(mag)) - 8)
    return ~((got - model).abs() <= half + slack)


def within_f32(got, model, slack):
    """fp32 outputs: |got - model| <= slack + one fp32 rounding of the result -> boolean tensor of violations"""
    return ~((got.double() - model).abs() <= slack + 2.0 ** -24 * model.abs())


# ------------------------------------------------------------------------------------------------------------------
# recipes (CPU float64 tensors of bf16 numbers; the same generator gives the same operands at every call)
# ------------------------------------------------------------------------------------------------------------------
def _gen(seed, device='cpu'):
    return torch.Generator(device=device).manual_seed(seed)


def ints(shape, lim, g):
    return torch.randint(-lim, lim + 1, shape, generator=g, device=g.device, dtype=torch.int8).double()


def gauss_bf16(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(BF).double()


def selection(n, k, g, per_row=1):
    """[n, k] with `per_row` entries +-2^e (e in [-2, 2]) per row, every column used (n * per_row >= k)"""
    assert n * per_row >= k and (n * per_row) % k == 0
    cols = torch.cat([torch.randperm(k, generator=g) for _ in range(n * per_row // k)]).view(per_row, n)
    w = torch.zeros(n, k, dtype=torch.float64)
    for r in range(per_row):
        e = torch.randint(-2, 3, (n,), generator=g).double()
        sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
        w[torch.arange(n), cols[r]] += sign * torch.exp2(e)
    assert int((w != 0).sum(1).min()) == per_row and bool((w != 0).any(0).all())
    return w


def sparse_cols(rows, cols, per_col, vals, g):
    """[rows, cols] with `per_col` entries drawn from `vals` in every column (distinct rows)"""
    w = torch.zeros(rows, cols, dtype=torch.float64)
    vals = torch.tensor(vals, dtype=torch.float64)
    for j in range(cols):
        r = torch.randperm(rows, generator=g)[:per_col]
        w[r, j] = vals[torch.randint(0, len(vals), (per_col,), generator=g)]
    return w


def recipe_i_linear(m, k, n, seed=0, device='cpu'):
    g = _gen(1000 + seed + k + 2 * n, device)
    return dict(x=ints((m, k), 8, g), w=ints((n, k), 4, g), bias=ints((n,), 8, g), aux=ints((m, n), 8, g))


def recipe_f_linear(m, k, n, seed=0, device='cpu'):
    """recipe I scaled by powers of two - weights / 64, biases / 8, aux / 4: as exact as recipe I (the granule moves with the
    scale), but the pre-activations are multiples of 1/64 of magnitude <= 10 with up to 10 significant bits: storing them rounds,
    and GELU is not saturated there - an activation taken at the unrounded pre-activation differs by more than the rule allows"""
    r = recipe_i_linear(m, k, n, seed + 17, device)
    return dict(x=r['x'], w=r['w'] / 64, bias=r['bias'] / 8, aux=r['aux'] / 4)


def recipe_s_linear(m, k, n, seed=0):
    g = _gen(2000 + seed + k + 2 * n)
    return dict(x=gauss_bf16((m, k), g), w=selection(n, k, g, 2 if n < k else 1), bias=None, aux=gauss_bf16((m, n), g))


def crafted_stats(m, g, delta_lim=2):
    """recipe B: -> (s [m, 128] integer, stats [m, 2] = mean | rstd) with xhat = (s - mean) rstd integer in [-delta_lim, delta_lim]"""
    mean = ints((m, 1), 8, g)
    rstd = torch.exp2(-torch.randint(0, 3, (m, 1), generator=g).double())
    delta = ints((m, 128), delta_lim, g)
    return mean + delta / rstd, torch.cat([mean, rstd], 1)


def recipe_b_ln(m, seed=0):
    """operands of sst_add_layernorm_bwd_bf16"""
    g = _gen(3000 + seed)
    s, st = crafted_stats(m, g)
    return dict(dy=ints((m, 128), 2, g), dy2=ints((m, 128), 1, g), s=s, st=st, w=ints((128,), 2, g))


def tail_params_i(seed=0):
    g = _gen(4000 + seed)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).float().double()   # noqa: E731  (fp32 parameters)
    return dict(w_out=ints((128, 128), 4, g), b_out=ints((128,), 8, g), w1=ints((256, 128), 4, g), b1=ints((256,), 8, g),
                w2=ints((128, 256), 4, g), b2=ints((128,), 8, g), n1w=1 + r(128, sc=0.2), n1b=r(128, sc=0.1),
                n2w=1 + r(128, sc=0.2), n2b=r(128, sc=0.1))


def tail_params_s(seed=0):
    """selection weights, zero biases; norm1 = +-1/4 xhat + an integer offset of magnitude 8 .. 16: y1 (bf16) is then a multiple
    of 2^-5 with 5 <= |y1| <= 19, h a multiple of 2^-7, and y1 + h[a] 2^ea + h[b] 2^eb an fp32 number (asserted)"""
    g = _gen(5000 + seed)
    z = lambda n: torch.zeros(n, dtype=torch.float64)   # noqa: E731
    sign = lambda n: torch.randint(0, 2, (n,), generator=g).double() * 2 - 1   # noqa: E731
    return dict(w_out=selection(128, 128, g), b_out=z(128), w1=selection(256, 128, g), b1=z(256), w2=selection(128, 256, g, 2),
                b2=z(128), n1w=0.25 * sign(128), n1b=sign(128) * torch.randint(8, 17, (128,), generator=g).double(),
                n2w=1 + (torch.randn(128, generator=g) * 0.2).float().double(), n2b=(torch.randn(128, generator=g) * 0.1).float().double())


def tail_inputs_i(m, seed=0):
    g = _gen(6000 + seed)
    return ints((m, 128), 8, g), ints((m, 128), 8, g)


def tail_inputs_s(m, seed=0):
    g = _gen(7000 + seed)
    return gauss_bf16((m, 128), g), gauss_bf16((m, 128), g)


def recipe_b_tail(m, seed=0):
    """operands of a tail backward call: -> (dict of saved tensors / gradients, dict of parameters)"""
    g = _gen(8000 + seed)
    s2, st2 = crafted_stats(m, g)
    s1, st1 = crafted_stats(m, g)
    t = dict(dy2=ints((m, 128), 2, g), dy2p=ints((m, 128), 1, g), s2=s2, st2=st2, s1=s1, st1=st1, pre=ints((m, 256), 3, g))
    p = dict(w_out=selection(128, 128, g).t().contiguous(), w1=sparse_cols(256, 128, 3, (-1.0, 1.0), g),
             w2=sparse_cols(128, 256, 2, (-2.0, -1.0, 1.0, 2.0), g), n2w=ints((128,), 2, g), n1w=ints((128,), 1, g))
    return t, p
