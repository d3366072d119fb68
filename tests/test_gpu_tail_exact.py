"""GPU: both one-kernel encoder tails - csrc/layer_tail_bf16.hip (bf16.tail_fwd / tail_bwd) and csrc/layer_tail_x6.hip
(dense.encoder_tail_fwd / encoder_tail_bwd under matmul_mode_scope('f32x6')) - at EVERY token count of a range more than twice
a workgroup's, against the float64 models of tests/bf16_exact_ref.py with exact operands.

Forward.  Recipe I (integers): s1 and the mean of norm1 bit for bit.  Recipe S (selection weights, Gaussian inputs): pre and
h = ReLU(pre) bit for bit given the kernel's own y1, in the bf16 mode s2 as well (norm1's parameters make y1 a multiple of 2^-5,
asserted on the kernel's own y1; in the fp32 mode y1 has 24 significant bits and the three-term sum is compared by the rule).
Everything else: each stage's model is fed with the kernel's own stored input of that stage and compared element by element.
Slack of a product stage = the fp32 roundings of its accumulation, (number of additions) * 2^-24 * (sum of the element's absolute
terms): 128 + 2 (pre) and 256 + 3 (s2) additions in the bf16 mode, three times the products in the exact-split mode (three parts
of the fp32 operand, bf16-exact weights: 386 and 771).  GELU, LayerNorm: gelu_slack, ln_y_slack, ln_in_err, RSTD_REL there.
h = GELU(pre) is GELU of the STORED pre-activation in both modes (test_bf16_tail_gelu_acts_on_the_stored_pre_activation).

Backward.  Recipe B (crafted statistics, ReLU): ds2, dpre, ds1, d_o and the four LayerNorm parameter gradients bit for bit in
both modes; GELU once per mode: ds2 and norm2's parameter gradients exact, dpre by the rule with gelu_grad_slack.

Guards.  Inputs sit in taller buffers whose rows from m on are NaN, outputs in taller buffers of sentinels; the workspace behind
the launched workgroups' partial rows is a sentinel as well.  A token beyond m that reaches a column sum, a statistic or a valid
row shows as NaN.  The counts are prefixes of operands generated once, walked downwards so that a row turns NaN once."""
import contextlib

import pytest
import torch

import bf16_exact_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF = torch.bfloat16
SENTINEL = -12288.0
PAD = 3
EPS = 1e-5
NPOS = 144
FWD_OUT = (('s1', 128), ('st1', 2), ('y1', 128), ('pre', 256), ('h', 256), ('s2', 128), ('st2', 2), ('y2', 128), ('y2p', 128))
BWD_OUT = (('ds2', 128), ('dpre', 256), ('ds1', 128), ('d_o', 128))


class _Mode:
    def __init__(self, name):
        from sst_amd import _lib, bf16 as B, dense as D
        lib = _lib.load()
        self.name, self.bf16 = name, name == 'bf16'
        self.dtype = BF if self.bf16 else torch.float32
        self.ws_bytes = lib.sst_encoder_tail_bwd_bf16_workspace_bytes if self.bf16 else lib.sst_encoder_tail_bwd_workspace_bytes
        m = 1
        while self.ws_bytes(m + 1) == self.ws_bytes(1):      # the workspace grows by one partial row pair per workgroup
            m += 1
        self.rows_per_wg = m
        self.counts = 2 * m + 16
        self.scope = contextlib.nullcontext if self.bf16 else (lambda: D.matmul_mode_scope('f32x6'))
        self.pack = B.tail_pack if self.bf16 else D.encoder_tail_pack
        self.fwd = B.tail_fwd if self.bf16 else D.encoder_tail_fwd
        self.bwd = B.tail_bwd if self.bf16 else D.encoder_tail_bwd
        self.k_pre, self.k_s2 = (130, 259) if self.bf16 else (386, 771)

    def within(self, got, model, slack):
        return R.within_bf16(got, model, slack) if self.bf16 else R.within_f32(got, model, slack)


def test_workgroup_rows_are_what_the_kernels_state():
    assert _Mode('bf16').rows_per_wg == 128 and _Mode('bf16').counts == 272
    assert _Mode('f32').rows_per_wg == 64 and _Mode('f32').counts == 144


class _Checks:
    def __init__(self):
        self.labels, self.flags = [], []

    def add(self, label, bad):
        self.labels.append(label)
        self.flags.append(bad.any() if bad.dim() else bad)

    def equal(self, label, got, want):
        self.add(label, got.double() != want)

    def finish(self):
        bad = torch.stack(self.flags).cpu().tolist()
        failed = [lab for lab, b in zip(self.labels, bad) if b]
        assert not failed, f'{len(failed)} of {len(bad)} checks failed, first: {failed[:8]}, last: {failed[-3:]}'
        assert len(bad) > 0


class _Frames:
    """inputs: [M + PAD] rows, NaN from row m on; outputs: [M + PAD] rows of sentinels"""

    def __init__(self, inputs, outputs, rows):
        self.rows = rows
        self.inp = {}
        for name, t in inputs.items():
            buf = torch.full((rows + PAD,) + tuple(t.shape[1:]), float('nan'), dtype=t.dtype, device=DEV)
            buf[:rows] = t
            self.inp[name] = buf
        self.out = {name: torch.full((rows + PAD, c), SENTINEL, dtype=dt, device=DEV) for name, (c, dt) in outputs.items()}
        self.m = rows

    def at(self, m):
        """-> (input views, output views) of the first m rows; m only walks downwards"""
        assert m <= self.m
        for buf in self.inp.values():
            buf[m:self.m] = float('nan')
        self.m = m
        return {k: v[:m] for k, v in self.inp.items()}, {k: v[:m] for k, v in self.out.items()}

    def check_and_reset(self, ck, lab, m, names):
        for name in names:
            buf = self.out[name]
            ck.add(lab + (name, 'frame'), (buf[m:] != SENTINEL).any() | torch.isnan(buf[:m]).any())
            buf[:m] = SENTINEL


def _f32(p):
    return {k: v.to(DEV).float().contiguous() for k, v in p.items()}


def _pos(rows, seed):
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((NPOS + 2, 128), float('nan'), device=DEV)
    buf[1:NPOS + 1] = torch.randn(NPOS, 128, generator=g).to(DEV)
    idx = torch.randint(0, NPOS, (rows,), generator=g, dtype=torch.int32)
    idx[0], idx[1 % rows] = NPOS - 1, 0
    idx = idx.to(DEV)
    return buf[1:NPOS + 1], idx, buf[1:NPOS + 1].double()[idx.long()]


def _run_fwd(mode, fr, m, pk, pf, act, pos, save=True):
    inp, out = fr.at(m)
    names = [n for n, _ in FWD_OUT if (pos is not None or n != 'y2p') and (save or n not in ('s1', 's2'))]
    with mode.scope():
        return mode.fwd(inp['o'], inp['x'], pk, pf['b_out'], pf['b1'], pf['b2'], pf['n1w'], pf['n1b'], pf['n2w'], pf['n2b'], EPS, act,
                        save=save, pos=(pos[0], pos[1][:m]) if pos is not None else None, out={n: out[n] for n in names}), names


# ---- forward, recipe I ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,act,with_pos', [('bf16', 'relu', True), ('bf16', 'gelu', False), ('bf16', 'gelu', True),
                                               ('f32', 'relu', True), ('f32', 'gelu', False), ('f32', 'relu', False)])
def test_forward_integers_every_token_count(name, act, with_pos):
    mode = _Mode(name)
    M = mode.counts
    o, x = (t.to(DEV) for t in R.tail_inputs_i(M))
    p = {k: v.to(DEV) for k, v in R.tail_params_i().items()}
    pf = _f32(p)
    with mode.scope():
        pk = mode.pack(pf['w_out'], pf['w1'], pf['w2'])
    pos = _pos(M, 1) if with_pos else None
    tr = R.Trace()
    mod = R.tail_fwd(o, x, p, act, EPS, bf16=mode.bf16, tr=tr)
    R.assert_exact(tr, only=('s1.',))
    fr = _Frames(dict(o=o.to(mode.dtype), x=x.to(mode.dtype)),
                 {n: (c, torch.float32 if n.startswith('st') else mode.dtype) for n, c in FWD_OUT}, M)
    ck = _Checks()
    u = 2.0 ** -24
    for m in range(M, 0, -1):
        out, names = _run_fwd(mode, fr, m, pk, pf, act, pos)
        lab = (name, act, m)
        # norm1: the sum and its mean exactly, rstd and y1 by the rule
        ck.equal(lab + ('s1',), out['s1'], mod['s1'][:m])
        ck.equal(lab + ('mean1',), out['st1'][:, 0], mod['mean1'][:m])
        ck.add(lab + ('rstd1',), ~((out['st1'][:, 1].double() / mod['rstd1'][:m] - 1).abs() <= R.RSTD_REL))
        ck.add(lab + ('y1',), mode.within(out['y1'], mod['y1v'][:m], R.ln_y_slack(mod['xhat1'][:m], p['n1w'], mod['y1v'][:m])))
        # the stages behind it, each fed with the kernel's own stored input
        y1k, prek, hk = out['y1'].double(), out['pre'].double(), out['h'].double()
        prev = y1k @ p['w1'].t() + p['b1']
        pre_slack = mode.k_pre * u * (y1k.abs() @ p['w1'].abs().t() + p['b1'].abs())
        ck.add(lab + ('pre',), mode.within(out['pre'], prev, pre_slack))
        if act == 'relu':
            ck.equal(lab + ('h',), out['h'], torch.relu(prek))
        else:
            hv = R.gelu64(prek)
            ck.add(lab + ('h',), mode.within(out['h'], hv, R.gelu_slack(prek, hv)))
        s2v = hk @ p['w2'].t() + p['b2'] + y1k
        d2 = mode.k_s2 * u * (hk.abs() @ p['w2'].abs().t() + p['b2'].abs() + y1k.abs())
        ck.add(lab + ('s2',), mode.within(out['s2'], s2v, d2))
        # norm2 normalises the unrounded fp32 sum: in the fp32 mode that IS the stored s2; in the bf16 mode it is within d2 of s2v
        l2 = R.ln_fwd(s2v if mode.bf16 else out['s2'].double(), p['n2w'], p['n2b'], EPS, pos[2][:m] if with_pos else None,
                      bf16=mode.bf16)
        drow = d2.max(1, keepdim=True).values if mode.bf16 else torch.zeros((m, 1), dtype=torch.float64, device=DEV)
        s2v = s2v if mode.bf16 else out['s2'].double()
        ck.add(lab + ('mean2',), ~((out['st2'][:, 0].double() - l2['mean']).abs() <= drow[:, 0] + 128 * u * s2v.abs().mean(1)))
        ck.add(lab + ('rstd2',), ~((out['st2'][:, 1].double() / l2['rstd'] - 1).abs() <= R.RSTD_REL + 2 * drow[:, 0] * l2['rstd']))
        # unlike s1, s2 is no integer row: its mean carries the 128 fp32 additions of the row sum, and moves every centred value
        mean_err = l2['rstd'][:, None] * p['n2w'].abs() * (128 * u * s2v.abs().mean(1, keepdim=True))
        sl = R.ln_y_slack(l2['xhat'], p['n2w'], l2['yv'], R.ln_in_err(drow, l2['rstd'], p['n2w'], l2['xhat']) + mean_err)
        ck.add(lab + ('y2',), mode.within(out['y2'], l2['yv'], sl))
        if with_pos:
            ck.add(lab + ('y2p',), mode.within(out['y2p'], l2['ypv'], sl + u * l2['ypv'].abs()))
        fr.check_and_reset(ck, lab, m, names)
    ck.finish()


def test_bf16_tail_gelu_acts_on_the_stored_pre_activation():
    """The elementwise rule for h = GELU(pre) of the bf16 tail, fed with the kernel's own STORED pre: what csrc/dense_bf16.hip does
    ("the activation acts on the ROUNDED value so that the backward's derivative is taken at the point the forward used") and what
    the header of csrc/layer_tail_bf16.hip promises ("rounded to bf16 exactly where the launch-per-product sequence rounded it").

    The kernel used to take GELU at the fp32 pre-activation it holds in registers (`gelu_f(p0[r])`) and store the rounded one
    beside it: with recipe I at 272 tokens 3191 of 69632 elements of h (4.6 %) were further from GELU(stored pre) than half a
    bf16 step + gelu_slack, the largest by 25.6 half-steps (where GELU is small against its argument).  ReLU commutes with the
    rounding and never showed it.  Also: h and pre are bit for bit what sst_tall_linear_bf16 (GELU epilogue) stores for the
    tail's own y1 - the same gelu_f at the same value."""
    from sst_amd import bf16 as B
    m = 272
    o, x = (t.to(DEV) for t in R.tail_inputs_i(m))
    p = {k: v.to(DEV) for k, v in R.tail_params_i().items()}
    pf = _f32(p)
    out = B.tail_fwd(o.to(BF), x.to(BF), B.tail_pack(pf['w_out'], pf['w1'], pf['w2']), pf['b_out'], pf['b1'], pf['b2'], pf['n1w'],
                     pf['n1b'], pf['n2w'], pf['n2b'], EPS, 'gelu')
    prek = out['pre'].double()
    hv = R.gelu64(prek)
    slack = R.gelu_slack(prek, hv)
    bad = R.within_bf16(out['h'], hv, slack)
    half = torch.exp2(torch.floor(torch.log2((hv.abs() + slack).clamp_min(2.0 ** -126))) - 8)
    excess = float((((out['h'].double() - hv).abs() - slack) / half).max())
    share = float(bad.double().mean())
    print(f'h beyond half a bf16 step of GELU(stored pre): {int(bad.sum())} of {bad.numel()} elements ({share:.4f}), '
          f'largest error {excess:.2f} half-steps')
    assert not bool(bad.any()), (int(bad.sum()), bad.numel(), excess)
    h, pre = B.tall_linear(out['y1'], pf['w1'].to(BF), pf['b1'], B.EPI_GELU, want_pre=True)
    assert torch.equal(pre, out['pre']) and torch.equal(h, out['h'])


# ---- forward, recipe S ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['bf16', 'f32'])
def test_forward_selection_weights_every_token_count(name):
    mode = _Mode(name)
    M = mode.counts
    o, x = (t.to(DEV) for t in R.tail_inputs_s(M))
    p = {k: v.to(DEV) for k, v in R.tail_params_s().items()}
    pf = _f32(p)
    with mode.scope():
        pk = mode.pack(pf['w_out'], pf['w1'], pf['w2'])
    fr = _Frames(dict(o=o.to(mode.dtype), x=x.to(mode.dtype)),
                 {n: (c, torch.float32 if n.startswith('st') else mode.dtype) for n, c in FWD_OUT}, M)
    ck = _Checks()
    full = None
    for m in range(M, 0, -1):
        out, names = _run_fwd(mode, fr, m, pk, pf, 'relu', None)
        lab = (name, 'S', m)
        y1k, hk = out['y1'].double(), out['h'].double()
        if full is None:
            # the exactness condition on the kernel's OWN y1 and h, once: rows do not depend on m (checked below)
            tr = R.Trace()
            mod = R.tail_fwd(o, x, p, 'relu', EPS, bf16=mode.bf16, tr=tr, y1=y1k, h=hk)
            R.assert_exact(tr, only=('pre.',) + (('s2.',) if mode.bf16 else ()))
            full = dict(y1=out['y1'].clone(), pre=mod['pre'], h=mod['h'], s2=mod['s2'], s2v=mod['s2v'], s2_abs=mod['s2_abs'])
            assert bool((mod['h'] == 0).any()) and bool((mod['h'] > 0).any())
        ck.add(lab + ('y1 as at the full count',), out['y1'] != full['y1'][:m])
        ck.equal(lab + ('pre',), out['pre'], full['pre'][:m])
        ck.equal(lab + ('h',), out['h'], full['h'][:m])
        if mode.bf16:
            ck.equal(lab + ('s2',), out['s2'], full['s2'][:m])
        else:       # y1 + h[a] 2^ea + h[b] 2^eb with 24-bit terms: two fp32 additions (three with the zero bias)
            ck.add(lab + ('s2',), R.within_f32(out['s2'], full['s2v'][:m], 3 * 2.0 ** -24 * full['s2_abs'][:m]))
        fr.check_and_reset(ck, lab, m, names)
    ck.finish()


# ---- backward, recipe B --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,act,with_dy2p', [('bf16', 'relu', True), ('bf16', 'relu', False), ('bf16', 'gelu', True),
                                                ('f32', 'relu', True), ('f32', 'relu', False), ('f32', 'gelu', True)])
def test_backward_crafted_statistics_every_token_count(name, act, with_dy2p):
    mode = _Mode(name)
    M = mode.counts
    t, p = R.recipe_b_tail(M)
    t, p = {k: v.to(DEV) for k, v in t.items()}, {k: v.to(DEV) for k, v in p.items()}
    pf = _f32(p)
    with mode.scope():
        pk = mode.pack(pf['w_out'], pf['w1'], pf['w2'])
    tr = R.Trace()
    mod = R.tail_bwd(t['dy2'], t['dy2p'] if with_dy2p else None, t['s2'], t['st2'], t['pre'], t['s1'], t['st1'], p, act,
                     bf16=mode.bf16, tr=tr)
    R.assert_exact(tr, only=None if act == 'relu' else ('ds2.', 'dpre.acc'))
    sums = [mod[k].cumsum(0) for k in ('dn2w_rows', 'dn2b_rows', 'dn1w_rows', 'dn1b_rows')]
    fr = _Frames({k: t[k].to(torch.float32 if k.startswith('st') else mode.dtype) for k in t},
                 {n: (c, mode.dtype) for n, c in BWD_OUT}, M)
    dn = torch.full((4 + 2 * PAD, 128), SENTINEL, device=DEV)
    ws_floats = mode.ws_bytes(M) // 4
    ws = torch.full((ws_floats + 64,), SENTINEL, device=DEV)
    ck = _Checks()
    for m in range(M, 0, -1):
        inp, out = fr.at(m)
        with mode.scope():
            mode.bwd(inp['dy2'], inp['dy2p'] if with_dy2p else None, inp['s2'], inp['st2'], inp['pre'], inp['s1'], inp['st1'], pk,
                     pf['n1w'], pf['n2w'], act, out=dict(out, dn=dn[PAD:PAD + 4], ws=ws))
        lab = (name, act, with_dy2p, m)
        ck.equal(lab + ('ds2',), out['ds2'], mod['ds2'][:m])
        for i in range(2 if act == 'gelu' else 4):
            ck.equal(lab + ('dn', i), dn[PAD + i], sums[i][m - 1])
        if act == 'relu':
            for k in ('dpre', 'ds1', 'd_o'):
                ck.equal(lab + (k,), out[k], mod[k][:m])
        else:
            v = mod['dprev'][:m]
            slack = mod['a1'][:m].abs() * R.gelu_grad_slack(t['pre'][:m]) + 2.0 ** -24 * v.abs()
            ck.add(lab + ('dpre',), mode.within(out['dpre'], v, slack))
            ck.add(lab + ('finite',), ~(torch.isfinite(out['ds1'].float()).all() & torch.isfinite(dn[PAD:PAD + 4]).all()))
        used = 2 * (-(-m // mode.rows_per_wg)) * 256         # part2 | part1 of the launched workgroups
        ck.add(lab + ('workspace',), (ws[used:] != SENTINEL).any() | (dn[:PAD] != SENTINEL).any() | (dn[PAD + 4:] != SENTINEL).any())
        ws[:used] = SENTINEL
        fr.check_and_reset(ck, lab, m, [n for n, _ in BWD_OUT])
    ck.finish()


@pytest.mark.parametrize('name', ['bf16', 'f32'])
def test_no_tokens(name):
    """m = 0: the forward returns OK and writes nothing, the backward zeroes the four parameter gradients"""
    mode = _Mode(name)
    p = _f32(R.tail_params_i())
    with mode.scope():
        pk = mode.pack(p['w_out'], p['w1'], p['w2'])
        empty = torch.empty((0, 128), dtype=mode.dtype, device=DEV)
        frame = {n: torch.full((PAD, c), SENTINEL, dtype=torch.float32 if n.startswith('st') else mode.dtype, device=DEV)
                 for n, c in FWD_OUT[:-1]}
        mode.fwd(empty, empty, pk, p['b_out'], p['b1'], p['b2'], p['n1w'], p['n1b'], p['n2w'], p['n2b'], EPS, 'gelu',
                 out={n: v[:0] for n, v in frame.items()})
        assert all(bool((v == SENTINEL).all()) for v in frame.values())
        dn = torch.full((4 + 2 * PAD, 128), SENTINEL, device=DEV)
        st = torch.empty((0, 2), device=DEV)
        e256 = torch.empty((0, 256), dtype=mode.dtype, device=DEV)
        mode.bwd(empty, None, empty, st, e256, empty, st, pk, p['n1w'], p['n2w'], 'relu', out=dict(dn=dn[PAD:PAD + 4]))
    assert bool((dn[PAD:PAD + 4] == 0).all()) and bool((dn[:PAD] == SENTINEL).all()) and bool((dn[PAD + 4:] == SENTINEL).all())


# ---- the bf16 tail against the launch-per-product sequence, as a statement -----------------------------------------------------
@pytest.mark.parametrize('m', [1, 77, 272])
def test_bf16_tail_stores_what_the_launch_per_product_kernels_store(m):
    """'the same roundings at the same places' (tests/test_gpu_encoder_tail_bf16.py) for the stages proven exact: s1 under recipe I;
    pre, h and s2 under recipe S, each unfused kernel fed with the tail's own stored input of that stage"""
    from sst_amd import bf16 as B
    ck = _Checks()
    for recipe, inputs, params in (('I', R.tail_inputs_i, R.tail_params_i), ('S', R.tail_inputs_s, R.tail_params_s)):
        o, x = (t.to(DEV) for t in inputs(272))
        p = {k: v.to(DEV) for k, v in params().items()}
        tr = R.Trace()
        mod = R.tail_fwd(o, x, p, 'relu', EPS, tr=tr)
        pf = _f32(p)
        ob, xb = o[:m].to(BF).contiguous(), x[:m].to(BF).contiguous()
        out = B.tail_fwd(ob, xb, B.tail_pack(pf['w_out'], pf['w1'], pf['w2']), pf['b_out'], pf['b1'], pf['b2'], pf['n1w'], pf['n1b'],
                         pf['n2w'], pf['n2b'], EPS, 'relu')
        wo, w1, w2 = (pf[k].to(BF) for k in ('w_out', 'w1', 'w2'))
        if recipe == 'I':
            R.assert_exact(tr, only=('s1.',))
            _, s1, st1, _ = B.linear_add_ln(ob, wo, pf['b_out'], xb, pf['n1w'], pf['n1b'], EPS)
            ck.add((recipe, 's1'), (s1 != out['s1']) | (s1.double() != mod['s1'][:m]))
            ck.add((recipe, 'mean1'), st1[:, 0] != out['st1'][:, 0])
        else:
            tr = R.Trace()
            R.tail_fwd(o[:m], x[:m], p, 'relu', EPS, tr=tr, y1=out['y1'].double(), h=out['h'].double())
            R.assert_exact(tr, only=('pre.', 's2.'))
            h, pre = B.tall_linear(out['y1'], w1, pf['b1'], B.EPI_RELU, want_pre=True)
            ck.add((recipe, 'pre'), pre != out['pre'])
            ck.add((recipe, 'h'), h != out['h'])
            _, s2, _, _ = B.linear_add_ln(out['h'], w2, pf['b2'], out['y1'], pf['n2w'], pf['n2b'], EPS)
            ck.add((recipe, 's2'), s2 != out['s2'])
    ck.finish()
