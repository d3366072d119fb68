"""GPU: the linears and LayerNorm kernels of the reduced-precision mode (csrc/dense_bf16.hip tall_linear_bf16_k - three shapes, seven
epilogues, both workgroup sizes; add_ln_fwd_bf16_k / add_ln_bwd_bf16_c128_k / cast_add_pos_bf16_k of csrc/dense.hip) against the
float64 models of tests/bf16_exact_ref.py with EXACT operands: a correct kernel returns the model bit for bit, so a truncating
store, an activation taken at the unrounded pre-activation, a residual added behind the rounding, a wrong statistic, a dropped or
doubled k-step or a mis-masked row is a hard mismatch.  Every `torch.equal`-class comparison has `assert_exact` in front of it.

Where no exactness argument exists (GELU, x GELU', rstd, the LayerNorm outputs) the kernel's element is compared with the model's,
element by element: half a bf16 step of the model value + a slack that is derived in tests/bf16_exact_ref.py from what the code
states (gelu_slack, gelu_grad_slack, ln_y_slack, RSTD_REL) - never scaled by a tensor's maximum, never taken from the kernel.

Token counts: every m in 1 .. 49 (rows_per_wave = 16: the second tile of the 32-row step is masked, its loads clamped), and per
instantiation the smallest m at which a wave walks 48, 64 and 80 rows (second step with one tile / two full steps / three steps,
the prefetch issued twice), found by bisection in the library's own partition (sst_tall_linear_bf16_partition).

Buffers: x is a column view of a 384-wide tensor, aux_in a column view with its own stride; every input sits in a taller buffer
whose other rows (and columns) are NaN, every output in a taller buffer of sentinels; the positional table has NaN guard rows."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import bf16_exact_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BF = torch.bfloat16
SHAPES = [(128, 128), (128, 256), (256, 128)]
SMALL = list(range(1, 50))
SENTINEL = -12288.0            # a bf16 number no test produces
PAD = 3
EPS = 1e-5
NPOS = 144
LN_LARGE = 4099                # no multiple of the 8 / 64 rows a block of the LayerNorm kernels takes per pass


# ---- the library's partition ---------------------------------------------------------------------------------------------------
def _partition(m, k, n, ln=False):
    from sst_amd import _lib
    b, r = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.load().sst_tall_linear_bf16_partition(m, k, n, int(ln), ctypes.byref(b), ctypes.byref(r)),
               'sst_tall_linear_bf16_partition')
    return b.value, r.value


def _waves_per_workgroup():
    """32768 rows are 16 rows for each wave of 256 eight-wave or 512 four-wave workgroups"""
    m = 1 << 15
    b, r = _partition(m, 128, 256)
    assert r == 16 and m % (b * r) == 0
    return m // (b * r)


def _walk_sizes(k, n, ln=False):
    """the smallest m at which a wave walks 48, 64, 80 rows (rows per wave never shrinks as m grows)"""
    sizes = []
    for rows in (48, 64, 80):
        lo, hi = 1, 1 << 22
        assert _partition(hi, k, n, ln)[1] >= rows
        while lo < hi:
            mid = (lo + hi) // 2
            if _partition(mid, k, n, ln)[1] >= rows:
                hi = mid
            else:
                lo = mid + 1
        sizes.append(lo)
    return sizes


def test_token_counts_follow_the_partition():
    """what the other tests rely on: at these sizes a wave walks exactly 48 / 64 / 80 rows, one row fewer gives one tile fewer,
    the last wave with rows has one row, trailing waves have none; below 50 rows a wave has one 16-row tile"""
    wpw = _waves_per_workgroup()
    assert wpw == (8 if os.environ.get('SST_AMD_BF16_LINEAR_WAVES') == '8' else 4)
    for k, n, ln in [(k, n, False) for k, n in SHAPES] + [(128, 128, True), (256, 128, True)]:
        assert all(_partition(m, k, n, ln)[1] == 16 for m in SMALL)
        for rows, m in zip((48, 64, 80), _walk_sizes(k, n, ln)):
            b, r = _partition(m, k, n, ln)
            assert r == rows and _partition(m - 1, k, n, ln)[1] == rows - 16
            assert m % 16 == 1 and -(-m // r) < b * wpw


# ---- buffers -------------------------------------------------------------------------------------------------------------------
def _framed(t, ld=None, col=0):
    """t [m, c] as a view inside a taller (and, with ld, wider) buffer of NaN"""
    m, c = t.shape
    big = torch.full((m + 2 * PAD, ld or c), float('nan'), dtype=t.dtype, device=DEV)
    big[PAD:PAD + m, col:col + c] = t
    return big[PAD:PAD + m, col:col + c]


class _Out:
    """an output view inside a taller (and, with ld, wider) buffer of sentinels; flags(): something outside the view changed |
    a NaN inside it"""

    def __init__(self, m, c, dtype=BF, ld=None, col=0):
        self.big = torch.full((m + 2 * PAD, ld or c), SENTINEL, dtype=dtype, device=DEV)
        self.view = self.big[PAD:PAD + m, col:col + c]
        self.m, self.c, self.col = m, c, col

    def flags(self):
        nan = torch.isnan(self.view).any()
        rest = self.big.clone()
        rest[PAD:PAD + self.m, self.col:self.col + self.c] = SENTINEL
        return (rest != SENTINEL).any() | nan


class _Checks:
    """device-side verdicts, read once at the end"""

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
        assert not failed, f'{len(failed)} of {len(bad)} checks failed, first: {failed[:8]}'
        assert len(bad) > 0


def _dev(t, dtype=BF):
    return t.to(DEV).to(dtype)


def _pos(m, seed):
    """-> (table view [NPOS, 128] fp32 between NaN guard rows, index int32 [m] with 0 and NPOS - 1, the gathered rows in float64)"""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((NPOS + 2, 128), float('nan'), device=DEV)
    buf[1:NPOS + 1] = torch.randn(NPOS, 128, generator=g).to(DEV)
    idx = torch.randint(0, NPOS, (m,), generator=g, dtype=torch.int32)
    idx[0], idx[-1] = NPOS - 1, 0
    idx = idx.to(DEV)
    return buf[1:NPOS + 1], idx, buf[1:NPOS + 1].double()[idx.long()]


# ---- sst_tall_linear_bf16 ------------------------------------------------------------------------------------------------------
def _linear_cases(ck, k, n, r, sizes, tag):
    """every epilogue at every m of `sizes` (prefixes of the operands r, float64 on the device) against the model"""
    from sst_amd import bf16 as B
    xs, w, bias, auxs = r['x'], r['w'], r['bias'], r['aux']
    wd, bd = w.to(BF).contiguous(), (bias.float() if bias is not None else None)
    tr = R.Trace()
    models = {}
    for epi in range(6):
        if bias is None and epi == R.EPI_ADD:
            continue      # recipe S: acc + a Gaussian aux is not claimed
        models[epi] = R.linear(xs, w, bias, epi, auxs, tr=tr)
    R.assert_exact(tr)
    no_bias = R.linear(xs, w, None, R.EPI_BIAS, tr=tr)
    for m in sizes:
        x = _framed(xs[:m].to(BF), 384, 384 - k)
        aux = _framed(auxs[:m].to(BF), n + 24, 8)
        assert x.stride(0) == 384 and aux.stride(0) == n + 24
        for epi, mod in models.items():
            lab = (tag, k, n, m, epi)
            y = _Out(m, n, ld=n + 16, col=8)
            if epi in (R.EPI_GELU, R.EPI_RELU):
                pre = _Out(m, n, ld=n + 8, col=0)
                B.tall_linear(x, wd, bd, epi, want_pre=True, out=y.view, pre_out=pre.view)
                ck.equal(lab + ('pre',), pre.view, mod['pre'][:m])
                ck.add(lab + ('pre frame',), pre.flags())
            else:
                B.tall_linear(x, wd, bd, epi, aux_in=aux if epi >= R.EPI_MUL_GELU_GRAD else None, out=y.view)
            if epi == R.EPI_GELU:
                v = mod['v'][:m]
                ck.add(lab + ('gelu',), R.within_bf16(y.view, v, R.gelu_slack(mod['pre'][:m], v)))
            elif epi == R.EPI_MUL_GELU_GRAD:
                v = mod['v'][:m]
                slack = mod['acc'][:m].abs() * R.gelu_grad_slack(auxs[:m]) + 2.0 ** -24 * v.abs()
                ck.add(lab + ('mul_gelu_grad',), R.within_bf16(y.view, v, slack))
            else:
                ck.equal(lab + ('y',), y.view, mod['y'][:m])
            ck.add(lab + ('frame',), y.flags())
        if bias is not None:
            y = _Out(m, n)
            B.tall_linear(x, wd, None, R.EPI_BIAS, out=y.view)
            ck.equal((tag, k, n, m, 'no bias'), y.view, no_bias['y'][:m])
            ck.add((tag, k, n, m, 'no bias frame'), y.flags())


def _on_dev(r):
    return {key: (v.to(DEV) if v is not None else None) for key, v in r.items()}


@pytest.mark.parametrize('k,n', SHAPES)
def test_linear_epilogues_every_small_token_count(k, n):
    ck = _Checks()
    _linear_cases(ck, k, n, _on_dev(R.recipe_i_linear(SMALL[-1], k, n)), SMALL, 'I')
    # pre-activations that are no bf16 numbers where GELU is not saturated: shows an activation taken at the unrounded value
    _linear_cases(ck, k, n, _on_dev(R.recipe_f_linear(SMALL[-1], k, n)), SMALL, 'F')
    if n >= k:      # selection weights: Gaussian bf16 inputs, every bit pattern of a stored value is the input's
        _linear_cases(ck, k, n, _on_dev(R.recipe_s_linear(SMALL[-1], k, n)), SMALL, 'S')
    ck.finish()


@pytest.mark.parametrize('k,n', SHAPES)
def test_linear_epilogues_second_and_third_step(k, n):
    ck = _Checks()
    for m in _walk_sizes(k, n):
        _linear_cases(ck, k, n, R.recipe_i_linear(m, k, n, device=DEV), [m], 'I')
    ck.finish()


# ---- sst_tall_linear_ln_bf16 ---------------------------------------------------------------------------------------------------
def _ln_params(seed):
    g = torch.Generator().manual_seed(seed)
    return (1 + 0.2 * torch.randn(128, generator=g)).to(DEV), (0.1 * torch.randn(128, generator=g)).to(DEV)


def _check_ln_outputs(ck, lab, mod, m, y, s, st, yp, in_err=0.0):
    """s, mean: bit-exact (callers assert exactness); rstd, y, y + pos: the elementwise rule"""
    if s is not None:
        ck.equal(lab + ('sum',), s, mod['s'][:m])
    ck.equal(lab + ('mean',), st[:, 0], mod['mean'][:m])
    ck.add(lab + ('rstd',), ~((st[:, 1].double() / mod['rstd'][:m] - 1).abs() <= R.RSTD_REL))
    slack = R.ln_y_slack(mod['xhat'][:m], mod['w'], mod['yv'][:m], in_err)
    ck.add(lab + ('y',), R.within_bf16(y, mod['yv'][:m], slack))
    if yp is not None:
        ck.add(lab + ('y + pos',), R.within_bf16(yp, mod['ypv'][:m], slack + 2.0 ** -24 * mod['ypv'][:m].abs()))


def _linear_ln_cases(ck, k, r, sizes):
    from sst_amd import bf16 as B
    xs, w, bias, res = r['x'], r['w'], r['bias'], r['aux']
    wd, bd = w.to(BF).contiguous(), bias.float()
    lw, lb = _ln_params(k)
    for m in sizes:
        table, idx, rows = _pos(m, m + k)
        x = _framed(xs[:m].to(BF), 384, 384 - k)
        rs = _framed(res[:m].to(BF))
        for with_bias in (True, False):
            tr = R.Trace()
            lin = R.linear(xs[:m], w, bias if with_bias else None, R.EPI_ADD, res[:m], tr=tr)
            mod = R.ln_fwd(lin['v'], lw.double(), lb.double(), EPS, rows, tr=tr)
            mod['w'] = lw.double()
            R.assert_exact(tr)
            for with_pos in (True, False):
                lab = ('ln', k, m, with_bias, with_pos)
                o = dict(y=_Out(m, 128), s=_Out(m, 128), stats=_Out(m, 2, torch.float32))
                if with_pos:
                    o['yp'] = _Out(m, 128)
                y, s, st, yp = B.linear_add_ln(x, wd, bd if with_bias else None, rs, lw, lb, EPS, pos=(table, idx) if with_pos else None,
                                               out={key: v.view for key, v in o.items()})
                _check_ln_outputs(ck, lab, mod, m, y, s, st, yp)
                for key, v in o.items():
                    ck.add(lab + (key, 'frame'), v.flags())
                if with_pos and with_bias:        # without the stored sum: the same y, bit for bit
                    y2, s2, _, yp2 = B.linear_add_ln(x, wd, bd, rs, lw, lb, EPS, save_sum=False, pos=(table, idx))
                    assert s2 is None
                    ck.add(lab + ('save_sum=False',), (y2 != y).any() | (yp2 != yp).any())


@pytest.mark.parametrize('k', [128, 256])
def test_linear_layernorm_epilogue_every_small_token_count(k):
    ck = _Checks()
    _linear_ln_cases(ck, k, _on_dev(R.recipe_i_linear(SMALL[-1], k, 128)), SMALL)
    ck.finish()


@pytest.mark.parametrize('k', [128, 256])
def test_linear_layernorm_epilogue_second_and_third_step(k):
    ck = _Checks()
    for m in _walk_sizes(k, 128, True):
        _linear_ln_cases(ck, k, R.recipe_i_linear(m, k, 128, device=DEV), [m])
    ck.finish()


# ---- the 8-wave instantiation --------------------------------------------------------------------------------------------------
def test_cases_of_this_process_workgroup_size():
    """the small counts and the three large sizes of one shape at the workgroup size THIS process runs (4 waves; 8 in the child of
    the next test, which sets SST_TEST_REQUIRE_WAVES so that a variable the library ignores fails here)"""
    want = int(os.environ.get('SST_TEST_REQUIRE_WAVES', '8' if os.environ.get('SST_AMD_BF16_LINEAR_WAVES') == '8' else '4'))
    assert _waves_per_workgroup() == want
    ck = _Checks()
    k, n = 128, 256
    _linear_cases(ck, k, n, _on_dev(R.recipe_i_linear(SMALL[-1], k, n)), SMALL, 'I')
    for m in _walk_sizes(k, n):
        assert _partition(m, k, n)[0] * want * _partition(m, k, n)[1] >= m
        _linear_cases(ck, k, n, R.recipe_i_linear(m, k, n, device=DEV), [m], 'I')
    _linear_ln_cases(ck, 256, _on_dev(R.recipe_i_linear(SMALL[-1], 256, 128)), SMALL[::3])
    ck.finish()


def test_eight_wave_instantiation_in_a_fresh_process():
    """NTH = 512 is chosen once per process by SST_AMD_BF16_LINEAR_WAVES=8: one child runs the test above with it"""
    env = dict(os.environ, SST_AMD_BF16_LINEAR_WAVES='8', SST_TEST_REQUIRE_WAVES='8')
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-p', 'no:cacheprovider', '-k',
                        'test_cases_of_this_process_workgroup_size'], env=env, capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and '1 passed' in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# ---- add_layernorm forward / backward, cast_add_pos (csrc/dense.hip) ------------------------------------------------------------
def _add_ln_fwd(x, res, w, b, y, s, stats, pos, yp):
    from sst_amd import _lib
    m, c = x.shape
    rc = _lib.load().sst_add_layernorm_fwd_bf16(_lib.ptr(x), _lib.ptr(res), _lib.ptr(w), _lib.ptr(b), m, c, EPS, _lib.ptr(y), _lib.ptr(s),
                                                _lib.ptr(stats), _lib.ptr(pos[0]) if pos else None, _lib.ptr(pos[1]) if pos else None,
                                                _lib.ptr(yp), _lib.stream_ptr())
    _lib.check(rc, 'sst_add_layernorm_fwd_bf16')


def test_add_layernorm_forward_every_token_count():
    """x even integers up to 254, the residual integers up to 127: the sum is an integer up to 381 - an fp32 number but above 256
    no bf16 number, so the stored sum really rounds; the mean (128 integers / 128) is exact"""
    g = torch.Generator().manual_seed(5)
    mx = LN_LARGE
    xs, rs = (2 * R.ints((mx, 128), 127, g)).to(DEV), R.ints((mx, 128), 127, g).to(DEV)
    lw, lb = _ln_params(9)
    tr = R.Trace()
    tr.value('sum', xs + rs)
    full = R.ln_fwd(xs + rs, lw.double(), lb.double(), EPS, tr=tr)
    R.assert_exact(tr)
    assert bool((full['s'] != xs + rs).any())
    ck = _Checks()
    for m in SMALL + [LN_LARGE]:
        table, idx, rows = _pos(m, m)
        mod = R.ln_fwd((xs + rs)[:m], lw.double(), lb.double(), EPS, rows)
        mod['w'] = lw.double()
        x, res = _framed(xs[:m].to(BF)), _framed(rs[:m].to(BF))
        o = dict(y=_Out(m, 128), s=_Out(m, 128), stats=_Out(m, 2, torch.float32), yp=_Out(m, 128))
        _add_ln_fwd(x, res, lw, lb, o['y'].view, o['s'].view, o['stats'].view, (table, idx), o['yp'].view)
        _check_ln_outputs(ck, ('add_ln', m), mod, m, o['y'].view, o['s'].view, o['stats'].view, o['yp'].view)
        for key, v in o.items():
            ck.add(('add_ln', m, key, 'frame'), v.flags())
        y2 = _Out(m, 128)
        _add_ln_fwd(x, res, lw, lb, y2.view, None, o['stats'].view, None, None)
        ck.add(('add_ln', m, 'without sum and pos'), (y2.view != o['y'].view).any() | y2.flags())
    ck.finish()


def test_add_layernorm_backward_crafted_statistics_every_token_count():
    """recipe B: dx (bf16), d(gamma), d(beta) bit for bit at every m; the column sums are prefix sums of the model's per-token terms"""
    from sst_amd import _lib
    lib = _lib.load()
    r = _on_dev(R.recipe_b_ln(LN_LARGE))
    wf = r['w'].float()
    ck = _Checks()
    for with_dy2 in (True, False):
        d = r['dy'] + r['dy2'] if with_dy2 else r['dy']
        tr = R.Trace()
        mod = R.ln_bwd(d, r['s'], r['st'][:, 0], r['st'][:, 1], r['w'], tr=tr)
        R.assert_exact(tr)
        cw, cb = mod['dw_rows'].cumsum(0), mod['db_rows'].cumsum(0)
        for m in SMALL + [LN_LARGE]:
            dy, dy2, s = (_framed(r[key][:m].to(BF)) for key in ('dy', 'dy2', 's'))
            st = _framed(r['st'][:m].float())
            dx, dw, db = _Out(m, 128), _Out(1, 128, torch.float32), _Out(1, 128, torch.float32)
            ws = _lib.workspace(lib.sst_add_layernorm_bwd_workspace_bytes(m, 128), torch.device(DEV))
            rc = lib.sst_add_layernorm_bwd_bf16(_lib.ptr(dy), _lib.ptr(dy2) if with_dy2 else None, _lib.ptr(s), _lib.ptr(st),
                                                _lib.ptr(wf), m, 128, _lib.ptr(dx.view), _lib.ptr(dw.view), _lib.ptr(db.view),
                                                _lib.ptr(ws), _lib.stream_ptr())
            _lib.check(rc, 'sst_add_layernorm_bwd_bf16')
            lab = ('ln_bwd', with_dy2, m)
            ck.equal(lab + ('dx',), dx.view, mod['dx'][:m])
            ck.equal(lab + ('dw',), dw.view[0], cw[m - 1])
            ck.equal(lab + ('db',), db.view[0], cb[m - 1])
            for o in (dx, dw, db):
                ck.add(lab + ('frame',), o.flags())
    ck.finish()


def test_cast_add_pos_every_token_count():
    """one fp32 addition (IEEE: the same bits as torch's on the same operands) and one RNE store: Gaussian fp32 and bf16 inputs,
    with and without the positional rows"""
    from sst_amd import _lib
    g = torch.Generator().manual_seed(6)
    xs = torch.randn(LN_LARGE, 128, generator=g).to(DEV)
    ck = _Checks()
    for m in SMALL + [LN_LARGE]:
        table, idx, _ = _pos(m, 3 * m)
        for dtype in (torch.float32, BF):
            x = _framed(xs[:m].to(dtype))
            for with_pos in (False, True):
                out = _Out(m, 128)
                rc = _lib.load().sst_cast_add_pos_bf16(_lib.ptr(x), int(dtype == BF), m, 128, _lib.ptr(table) if with_pos else None,
                                                       _lib.ptr(idx) if with_pos else None, _lib.ptr(out.view), _lib.stream_ptr())
                _lib.check(rc, 'sst_cast_add_pos_bf16')
                want = (x.float() + table[idx.long()]) if with_pos else x.float()
                lab = ('cast', m, str(dtype), with_pos)
                ck.add(lab, (out.view != want.to(BF)).any())
                ck.add(lab + ('frame',), out.flags())
    ck.finish()
