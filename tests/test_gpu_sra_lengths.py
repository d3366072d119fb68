"""GPU: the attention kernels at EVERY window length of every launch class (csrc/sra_attn.hip, csrc/sra_attn_bf16.hip).

The register-resident kernels pick their build from the launch's announced max_tokens (<= 4, 5, <= 7, 9 tiles of 16 tokens) and
each workgroup then picks a body from its own window's tile count; the LDS-staged kernels (impl 2) and the bf16 twins have
classes of their own.  tests/test_gpu_sra.py announces max(sizes) of short hand-picked lists; here every length 1..cap runs
inside the build of cap = 64, 80, 112 and 144, as a small launch (copies = 1: query-tile split on, no launch order) and as a
large one (LARGE_COPIES[cap] = 17, 13, 10, 8 copies: the fewest that put cap * copies windows of 8 heads past the 2048
workgroups below which the split is on - launch order on, split off, what a production frame is).  Caps 64, 80 and 112 run
at 8 copies too in (a): launch order AND split on.

a. every length against float64 (tests/sra_ref.py), per window.  The bar is F times the distance of the float32 restatement of
   the same formula from float64 on the same operands (E32, computed here at run time).  F was determined on the MI355X as
   twice the largest ratio of kernel distance to E32 over every (path, cap, copies, tensor), rounded up: the largest is 5.18
   (dk of the two-launch backward, d head_scale of the cosine backward), so F = 11.  The forward stays at 1.4 and the
   LDS-staged and generic backward below 2.7; the register-resident backward reaches 4 .. 5 because it recomputes P from the
   stored lse through the log2 domain and from scores rounded differently than the forward's (table and account in
   CHANGELOG.md).  Every case prints its ratios before it asserts.
b. exact routing: operands on which the forward is a pure gather (sra_ref.one_hot_case), every comparison ==.
c. nothing outside a window is read or written: the rows no window lists hold NaN in every operand and a sentinel bit pattern
   in every output buffer, and still hold it afterwards.  The forward and the cosine backward are called at the C entry
   points for this, with buffers allocated here (the Python wrappers allocate o, lse and r themselves); the wrappers run in (d).
d. the identity token list against rows_in_window_order, bit for bit, over the full sweep.
e. max_tokens is an inclusive bound: the windows of exactly `cap` tokens are computed (fp32: part of (a); bf16 here).
"""
import functools

import numpy as np
import pytest
import torch

import sra_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SCALE = 0.25
F = 11                       # kernel distance <= F * E32 (module docstring, CHANGELOG.md)
SENTINEL32 = 0x7FA5A5A5      # a NaN with a payload: a row that still holds it was not written, a written row is finite
SENTINEL16 = 0x7FA5          # the same for bf16
LARGE_COPIES = {64: 17, 80: 13, 112: 10, 144: 8}    # smallest copies with cap * copies * 8 heads / 4 > 2048 workgroups
assert all(cap * n * 2 > 2048 >= cap * (n - 1) * 2 for cap, n in LARGE_COPIES.items())


def _fill_sentinel(t):
    if t.dtype == torch.float32:
        t.view(torch.int32).fill_(SENTINEL32)
    elif t.dtype == torch.bfloat16:
        t.view(torch.int16).fill_(SENTINEL16)
    return t


def _holds_sentinel(t):
    if t.dtype == torch.float32:
        return t.view(torch.int32) == SENTINEL32
    return t.view(torch.int16) == SENTINEL16


def _sentinel_like(t):
    return _fill_sentinel(torch.empty_like(t))


def _forward(kind, q, k, v, plan, heads, scale_or_hs, impl=0):
    """the forward C entry point of `kind` (f32 | cos | bf16 | bf16_cos) with o and lse allocated and sentinel-filled here;
    argument lists as in sst_amd.kernels._sra_fwd / _sra_cos_fwd and sst_amd.bf16.sra_fwd / sra_cos_fwd"""
    from sst_amd import _lib
    lib, P = _lib.load(), _lib.ptr
    o = _sentinel_like(q)
    lse = _fill_sentinel(torch.empty((q.size(0), heads), dtype=torch.float32, device=q.device))
    head = (P(q), P(k), P(v), q.stride(0), k.stride(0), v.stride(0), plan.tok_ptr(impl), P(plan.winoff), P(plan.order),
            plan.n_windows, heads)
    tail = (P(o), o.stride(0), P(lse), _lib.stream_ptr())
    if kind == 'f32':
        rc = lib.sst_sra_attn_fwd_ord_f32(*head, float(scale_or_hs), plan.max_tokens, impl, *tail)
    elif kind == 'cos':
        rc = lib.sst_sra_attn_cos_fwd_f32(*head, P(scale_or_hs), plan.max_tokens, *tail)
    elif kind == 'bf16':
        rc = lib.sst_sra_attn_fwd_ord_bf16(*head, float(scale_or_hs), plan.max_tokens, *tail)
    else:
        rc = lib.sst_sra_attn_cos_fwd_bf16(*head, P(scale_or_hs), plan.max_tokens, *tail)
    _lib.check(rc, 'forward ' + kind)
    return o, lse


def _cosine_backward(kind, q, k, v, o, lse, do, plan, heads, hs, dq, dk, dv):
    """the cosine backward C entry point (cos | bf16_cos) with r allocated and sentinel-filled here -> r [rows, heads]"""
    from sst_amd import _lib
    lib, P = _lib.load(), _lib.ptr
    r = _fill_sentinel(torch.empty((q.size(0), heads), dtype=torch.float32, device=q.device))
    head = (P(q), P(k), P(v), P(o), P(do), P(lse), q.stride(0), k.stride(0), v.stride(0), o.stride(0), do.stride(0),
            plan.tok_ptr(0), P(plan.winoff), P(plan.order), plan.n_windows)
    tail = (heads, P(hs), plan.max_tokens, P(dq), P(dk), P(dv), dq.stride(0), dk.stride(0), dv.stride(0), P(r), _lib.stream_ptr())
    if kind == 'cos':
        rc = lib.sst_sra_attn_cos_bwd_f32(*head, q.size(0), *tail)
    else:
        rc = lib.sst_sra_attn_cos_bwd_bf16(*head, *tail)
    _lib.check(rc, 'cosine backward ' + kind)
    return r


class _Layout(object):
    """a sweep on the device: token list, the window of every token-list position, the unreferenced rows, the plan"""

    def __init__(self, sizes, tok, off, rows, max_tokens, rows_in_window_order=False):
        from sst_amd import kernels as K
        self.sizes, self.tok, self.off, self.rows = np.asarray(sizes), tok, off, rows
        self.n_win, self.m = len(sizes), int(off[-1])
        self.tok_d = torch.from_numpy(tok.astype(np.int64)).to(DEV)
        self.win_of_pos = torch.repeat_interleave(torch.arange(self.n_win), torch.from_numpy(self.sizes)).to(DEV)
        self.idle = torch.from_numpy(sra_ref.unreferenced_rows(tok, rows)).to(DEV)
        self.plan = K.WindowPlan(torch.from_numpy(tok).to(DEV), torch.from_numpy(off).to(DEV), self.n_win, self.m, max_tokens,
                                 rows_in_window_order=rows_in_window_order)

    def assert_launch_size(self, heads, copies, cap):
        """copies = 1 is a small launch: query-tile split on (at most 2048 workgroups), no launch order.  LARGE_COPIES[cap] is
        a large one: launch order on, split off (more than 2048 workgroups).  Anything between has the order and the split"""
        wg = self.n_win * heads // 4
        if copies == 1:
            assert wg <= 2048 and self.plan.order is None, wg
        elif copies == LARGE_COPIES[cap]:
            assert wg > 2048 and self.plan.order is not None, wg
        else:
            assert wg <= 2048 and self.plan.order is not None, wg

    def per_window_max(self, per_row):
        """[rows] -> [n_win]: the largest value over the window's rows (NaN counts as infinite)"""
        e = torch.nan_to_num(per_row[self.tok_d], nan=float('inf'))
        return torch.zeros(self.n_win, dtype=e.dtype, device=DEV).scatter_reduce_(0, self.win_of_pos, e, 'amax')

    def describe(self, bad_windows):
        ts = sorted(set(int(self.sizes[w]) for w in bad_windows.nonzero().flatten().tolist()))
        return ', '.join(f't={t} (tiles {sra_ref.tiles(t)}, t%16 {t % 16})' for t in ts)

    def assert_every_length_compared(self, cap, compared):
        """compared: bool [n_win], the windows for which every compared quantity was a finite number held against its bar ->
        every length 1..cap and every tile count of the class is among them"""
        ts = self.sizes[compared.cpu().numpy()]
        assert set(ts.tolist()) == set(range(1, cap + 1)), 'a window length was not compared'
        per_tiles = np.bincount((ts + 15) // 16, minlength=sra_ref.tiles(cap) + 1)
        assert (per_tiles[1:] > 0).all() and len(per_tiles) == sra_ref.tiles(cap) + 1, (cap, per_tiles.tolist())

    def assert_untouched_and_written(self, outputs, what):
        """every unreferenced row of every output still holds the sentinel bit for bit; every referenced row is finite"""
        for name, t in outputs.items():
            assert bool(_holds_sentinel(t[self.idle]).all()), f'{what}: {name} was written outside the windows'
            finite = torch.isfinite(t[self.tok_d].float()).all(dim=1)
            if not bool(finite.all()):
                bad = torch.zeros(self.n_win, device=DEV).scatter_reduce_(0, self.win_of_pos, (~finite).float(), 'amax') > 0
                raise AssertionError(f'{what}: {name} has rows that are not finite (unwritten, or NaN was read): ' + self.describe(bad))


# ------------------------------------------------------------------------------------------------------------------
# a. + c.: every length against float64, nothing outside a window read or written
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _random_case(cap, copies, heads, cosine):
    """operands, layout, the float64 reference and the float32 restatement's distance from it: computed once per sweep and
    shared by every path (and left unchanged)"""
    sizes, tok, off, rows = sra_ref.length_sweep(cap, copies, seed=cap * 10 + copies)
    lay = _Layout(sizes, tok, off, rows, cap)
    g = torch.Generator(device=DEV).manual_seed(cap * 100 + copies * 10 + heads)
    c = heads * 16
    q, k = (torch.randn(rows, c, generator=g, device=DEV) * 1.5 for _ in range(2))
    v, do = (torch.randn(rows, c, generator=g, device=DEV) for _ in range(2))
    hs = None
    if cosine:   # rows of very different norms, temperatures in [0.05, 0.55] (tests/test_gpu_cosine.py)
        rs = torch.rand(rows, 1, generator=g, device=DEV).mul(3).add(0.1)
        q, k = q * rs, k * rs
        hs = 1.0 / (torch.rand(heads, generator=g, device=DEV) * 0.5 + 0.05)
    for t in (q, k, v, do):
        t[lay.idle] = float('nan')
    ref = sra_ref.window_attention(q, k, v, tok, off, heads, SCALE, torch.float64, cosine_scale=hs, grad_o=do)
    low = sra_ref.window_attention(q, k, v, tok, off, heads, SCALE, torch.float32, cosine_scale=hs, grad_o=do)
    e32 = {}
    for n in ref:
        d = (low[n].double() - ref[n]).abs()
        e32[n] = float((d if n == 'dscale' else d[lay.tok_d]).max())
        assert 0.0 < e32[n] < 1e-3, (n, e32[n])
    return dict(lay=lay, q=q, k=k, v=v, do=do, hs=hs, ref=ref, e32=e32)


def _launch(path, case, heads):
    """one forward and one backward launch of `path` -> dict of output tensors (kernel-written buffers the test pre-filled)"""
    from sst_amd import kernels as K
    q, k, v, do, hs, plan = case['q'], case['k'], case['v'], case['do'], case['hs'], case['lay'].plan
    dq, dk, dv = (_sentinel_like(q) for _ in range(3))
    if path == 'cosine':
        assert K.cosine_kernels_ok(plan, heads)
        o, lse = _forward('cos', q, k, v, plan, heads, hs)
        r = _cosine_backward('cos', q, k, v, o, lse, do, plan, heads, hs, dq, dk, dv)
        return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv, r=r)
    impl = int(path[-1])
    o, lse = _forward('f32', q, k, v, plan, heads, SCALE, impl)
    K._sra_bwd(q, k, v, o, lse, do, plan, heads, SCALE, impl, dq, dk, dv)
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)


def _length_cases():
    cases = []
    for cosine in (False, True):
        paths = ['cosine'] if cosine else ['impl0', 'impl3', 'impl2']
        for cap in sra_ref.CAPS:
            for copies in sorted({1, 8, LARGE_COPIES[cap]}):
                cases += [(p, cap, copies, 8) for p in paths]
            if cap == 144:   # the generic kernel once; head-group counts of 3 and 1
                cases += [('impl1', 144, 1, 8)] if not cosine else []
                cases += [(p, 144, 1, h) for h in (12, 4) for p in paths + ([] if cosine else ['impl1'])]
    return cases


@pytest.mark.parametrize('path,cap,copies,heads', _length_cases())
def test_every_length_of_every_class_against_float64(path, cap, copies, heads):
    case = _random_case(cap, copies, heads, path == 'cosine')
    lay, ref, e32 = case['lay'], case['ref'], case['e32']
    lay.assert_launch_size(heads, copies, cap)
    out = _launch(path, case, heads)
    # c. (the generic backward accumulates dK / dV with atomics into buffers it clears itself: finiteness only)
    checked = {n: t for n, t in out.items() if not (path == 'impl1' and n in ('dk', 'dv'))}
    lay.assert_untouched_and_written(checked, path)
    if path == 'impl1':
        assert bool(torch.isfinite(out['dk'][lay.tok_d]).all() and torch.isfinite(out['dv'][lay.tok_d]).all())
    # a.
    failures = []
    compared = torch.ones(lay.n_win, dtype=torch.bool, device=DEV)      # windows whose every error below is a finite number
    for name in ('o', 'lse', 'dq', 'dk', 'dv'):
        err = lay.per_window_max((out[name].double() - ref[name]).abs().amax(dim=1))
        compared &= torch.isfinite(err)
        ratio = float(err.max()) / e32[name]
        print(f'ratio {path} cap {cap} copies {copies} heads {heads} {name}: {ratio:.2f} (E32 {e32[name]:.2e})')
        if ratio > F:
            failures.append(f'{name}: {float(err.max()):.3e} > {F} * {e32[name]:.3e} at ' + lay.describe(err > F * e32[name]))
    if path == 'cosine':   # every window's share of d head_scale: the sum of r over its rows, divided by the scale
        r = out['r'][lay.tok_d].double()
        share = torch.zeros(lay.n_win, heads, dtype=torch.float64, device=DEV).index_add_(0, lay.win_of_pos, r) / case['hs'].double()
        err = torch.nan_to_num((share - ref['dscale']).abs().amax(dim=1), nan=float('inf'))
        compared &= torch.isfinite(err)
        ratio = float(err.max()) / e32['dscale']
        print(f'ratio {path} cap {cap} copies {copies} heads {heads} dscale: {ratio:.2f} (E32 {e32["dscale"]:.2e})')
        if ratio > F:
            failures.append(f'dscale: {float(err.max()):.3e} > {F} * {e32["dscale"]:.3e} at ' + lay.describe(err > F * e32['dscale']))
    assert not failures, f'{path} cap {cap} copies {copies} heads {heads}: ' + '; '.join(failures)
    lay.assert_every_length_compared(cap, compared)     # all of them held against F * E32 just above


# ------------------------------------------------------------------------------------------------------------------
# b. exact routing (with c. on the same launches)
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _one_hot_case(cap, copies, cosine):
    sizes = sra_ref.length_sweep(cap, copies, seed=cap + copies)[0]
    case = sra_ref.one_hot_case(sizes, 8, seed=cap * 3 + copies, cosine=cosine)
    lay = _Layout(case['sizes'], case['tok'], case['off'], case['rows'], cap)
    q, k, v = (case[n].to(DEV) for n in ('q', 'k', 'v'))
    g = torch.Generator(device=DEV).manual_seed(cap)
    do = torch.randn(q.shape, generator=g, device=DEV).to(torch.bfloat16).float()
    for t in (q, k, v, do):
        t[lay.idle] = float('nan')
    src = case['src'].to(DEV)
    want = torch.stack([v[src[:, h], h * 16:(h + 1) * 16] for h in range(8)], 1).reshape(lay.m, 128)   # by token-list position
    hs = case['head_scale'].to(DEV) if cosine else None
    return dict(lay=lay, q=q, k=k, v=v, do=do, hs=hs, want=want, max_score=case['max_score'].to(DEV))


@pytest.mark.parametrize('path,cap,copies', [(p, cap, copies) for cap in sra_ref.CAPS for copies in (1, LARGE_COPIES[cap])
                                             for p in ('impl0', 'impl2', 'impl1', 'bf16', 'cosine', 'bf16_cosine')])
def test_one_hot_operands_are_routed_exactly(path, cap, copies):
    """o[i] == v[pi(i)] bit for bit at every length of every class: the transposed 4 x 4 key-slot grid, the skipped k-steps of
    the last tile, the -inf mask, the repeated-last-token padding, the q_row selection across 64-position registers, the
    split's query-tile dealing and the bf16 rounding of P have no tolerance to hide in"""
    from sst_amd import bf16 as B
    from sst_amd import kernels as K
    cosine = path.endswith('cosine')
    case = _one_hot_case(cap, copies, cosine)
    lay, hs, plan = case['lay'], case['hs'], case['lay'].plan
    lay.assert_launch_size(8, copies, cap)
    low = path.startswith('bf16')
    q, k, v, do = ((case[n].to(torch.bfloat16) if low else case[n]) for n in ('q', 'k', 'v', 'do'))
    dq, dk, dv = (_sentinel_like(q) for _ in range(3))
    extra = {}
    if cosine:
        kind = 'bf16_cos' if low else 'cos'
        o, lse = _forward(kind, q, k, v, plan, 8, hs)
        extra['r'] = _cosine_backward(kind, q, k, v, o, lse, do, plan, 8, hs, dq, dk, dv)
    elif low:
        o, lse = _forward('bf16', q, k, v, plan, 8, SCALE)
        B.sra_bwd(q, k, v, o, lse, do, plan, 8, SCALE, dq, dk, dv)
    else:
        o, lse = _forward('f32', q, k, v, plan, 8, SCALE, int(path[-1]))
        K._sra_bwd(q, k, v, o, lse, do, plan, 8, SCALE, int(path[-1]), dq, dk, dv)
    got = o[lay.tok_d].float()
    wrong = (got != case['want']).any(dim=1)
    wrong_w = torch.zeros(lay.n_win, device=DEV).scatter_reduce_(0, lay.win_of_pos, wrong.float(), 'amax') > 0
    assert not bool(wrong.any()), f'{path} cap {cap} copies {copies}: o != v[pi] at ' + lay.describe(wrong_w)
    # lse = max_score exactly in real arithmetic (the row sum is 1); the kernels form it as mx * ln 2: two roundings
    rel = ((lse[lay.tok_d].double() - case['max_score'][None, :]).abs() / case['max_score'][None, :]).amax(dim=1)
    rel_w = lay.per_window_max(torch.zeros(lay.rows, dtype=torch.float64, device=DEV).index_copy_(0, lay.tok_d, rel))
    assert float(rel_w.max()) <= 1e-6, f'{path} cap {cap} copies {copies}: lse != max score at ' + lay.describe(rel_w > 1e-6)
    # compared: the windows whose every o and lse value is a finite number that was held against v[pi] / the maximum score
    finite = torch.isfinite(got).all(dim=1) & torch.isfinite(lse[lay.tok_d]).all(dim=1)
    unfinished = torch.zeros(lay.n_win, device=DEV).scatter_reduce_(0, lay.win_of_pos, (~finite).float(), 'amax') > 0
    lay.assert_every_length_compared(cap, ~unfinished & ~wrong_w & (rel_w <= 1e-6))
    # The backward is deliberately NOT asserted exact on these operands: it recomputes P from the rounded lse, so P is
    # 1 +- 2e-4 there and dS = P (dP - D) is the rounding residue of two equal numbers.  It ran on the NaN-bordered operands:
    # it must have written every listed row with finite numbers and no other row.
    outs = dict(o=o, lse=lse, dq=dq, **extra)
    if path != 'impl1':
        outs.update(dk=dk, dv=dv)
    else:   # the generic backward accumulates dK / dV with atomics into buffers it clears itself: finiteness only
        assert bool(torch.isfinite(dk[lay.tok_d]).all() and torch.isfinite(dv[lay.tok_d]).all())
    lay.assert_untouched_and_written(outs, path)


# ------------------------------------------------------------------------------------------------------------------
# d. token list against rows in window order
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cap,copies', [(cap, copies) for cap in sra_ref.CAPS for copies in (1, LARGE_COPIES[cap])])
def test_identity_token_list_equals_rows_in_window_order(cap, copies):
    """the existing test_window_ordered_rows_need_no_token_list over the full sweep: with tok == arange(M) the kernels that take
    d_tok = NULL return the same bits as with the list - forward, one-pass and two-launch backward, cosine; through
    the Python wrappers, which choose the token pointer and allocate the outputs themselves"""
    from sst_amd import kernels as K
    sizes = sra_ref.length_sweep(cap, copies, seed=cap - copies)[0]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    m = int(off[-1])
    g = torch.Generator(device=DEV).manual_seed(cap + copies)
    qkv = torch.randn(m, 384, generator=g, device=DEV)
    do = torch.randn(m, 128, generator=g, device=DEV)
    hs = torch.linspace(2.0, 18.0, 8, device=DEV)
    q, k, v = qkv[:, :128], qkv[:, 128:256], qkv[:, 256:]
    outs = []
    for flag in (False, True):
        lay = _Layout(sizes, np.arange(m, dtype=np.int32), off, m, cap, rows_in_window_order=flag)
        lay.assert_launch_size(8, copies, cap)
        assert (lay.plan.tok_ptr(0) is None) == flag and (lay.plan.tok_ptr(3) is None) == flag
        assert lay.plan.tok_ptr(1) is not None and lay.plan.tok_ptr(2) is not None
        res = []
        o, lse = K._sra_fwd(q, k, v, lay.plan, 8, SCALE, 0)
        res += [o, lse]
        for impl in (0, 3):
            d = torch.zeros_like(qkv)
            K._sra_bwd(q, k, v, o, lse, do, lay.plan, 8, SCALE, impl, d[:, :128], d[:, 128:256], d[:, 256:])
            res.append(d)
        oc, lsec = K._sra_cos_fwd(q, k, v, lay.plan, 8, hs)
        d = torch.zeros_like(qkv)
        r = K._sra_cos_bwd(q, k, v, oc, lsec, do, lay.plan, 8, hs, d[:, :128], d[:, 128:256], d[:, 256:])
        res += [oc, lsec, d, r]
        assert all(bool(torch.isfinite(t).all()) for t in res)
        outs.append(res)
    for i, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a, b), f'output {i} differs between the token list and rows in window order'


# ------------------------------------------------------------------------------------------------------------------
# e. max_tokens is an inclusive upper bound
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cap', sra_ref.CAPS)
def test_windows_of_exactly_the_announced_size_are_computed(cap):
    """include/sst_amd.h: max_tokens must be an upper bound of every window of the call - a longer window is skipped by the
    register-resident kernels and picked up by no other.  The bound is inclusive: announce `cap` with windows of 1..cap and
    every row of every window comes back.  For the fp32 kernels that is part of (a), whose sweeps hold the window of exactly
    `cap` tokens and announce `cap`; here the bf16 kernels, forward and backward, on the same operands"""
    from sst_amd import bf16 as B
    case = _random_case(cap, 1, 8, False)
    lay, plan = case['lay'], case['lay'].plan
    assert plan.max_tokens == cap == int(lay.sizes.max()) and int((lay.sizes == cap).sum()) == 1
    qb, kb, vb, dob = (case[n].to(torch.bfloat16) for n in ('q', 'k', 'v', 'do'))
    dq, dk, dv = (_sentinel_like(qb) for _ in range(3))
    o, lse = _forward('bf16', qb, kb, vb, plan, 8, SCALE)
    B.sra_bwd(qb, kb, vb, o, lse, dob, plan, 8, SCALE, dq, dk, dv)
    lay.assert_untouched_and_written(dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv), 'bf16')
