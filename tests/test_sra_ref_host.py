"""CPU: the reference and the operand recipes of the attention length sweeps (tests/sra_ref.py).

* window_attention(float64) is the project's oracle (oracle/sst_oracle.sra_core, sra_core_backward) to 1e-12;
* the exact-routing operands keep their gap at every length 1..144 and a float32 softmax routes them exactly;
* the float32 restatement's distance from float64 on the four sweeps, printed: the figures the GPU bars multiply."""
import numpy as np
import pytest
import torch

import sra_ref
from oracle import sst_oracle


def _random_operands(rows, heads, seed, cosine=False):
    g = torch.Generator().manual_seed(seed)
    c = heads * 16
    q, k = torch.randn(rows, c, generator=g) * 1.5, torch.randn(rows, c, generator=g) * 1.5
    if cosine:
        rs = torch.rand(rows, 1, generator=g).mul(3).add(0.1)
        q, k = q * rs, k * rs
    return q, k, torch.randn(rows, c, generator=g), torch.randn(rows, c, generator=g)


def test_window_attention_float64_is_the_oracle():
    rng = np.random.default_rng(0)
    sizes = np.array([1, 2, 17, 64, 5, 144, 33, 100])
    tok, off, rows = sra_ref.token_list(sizes, rng)
    q, k, v, do = _random_operands(rows, 8, 1)
    got = sra_ref.window_attention(q, k, v, tok, off, 8, 0.25, torch.float64, grad_o=do, chunk=3)
    o, lse = sst_oracle.sra_core(q.numpy(), k.numpy(), v.numpy(), tok, off, 8, return_lse=True)
    dq, dk, dv = sst_oracle.sra_core_backward(q.numpy(), k.numpy(), v.numpy(), do.numpy(), tok, off, 8)
    for name, want in (('o', o), ('lse', lse), ('dq', dq), ('dk', dk), ('dv', dv)):
        err = float(np.abs(got[name].numpy() - want).max())
        assert err <= 1e-12 * max(1.0, float(np.abs(want).max())), (name, err)
    idle = sra_ref.unreferenced_rows(tok, rows)
    assert len(idle) == sra_ref.EXTRA_ROWS
    for name in ('o', 'lse', 'dq', 'dk', 'dv'):
        assert float(got[name][idle].abs().max()) == 0.0, name


def test_window_attention_never_reads_unreferenced_rows():
    sizes, tok, off, rows = sra_ref.length_sweep(64, 1, 3)
    q, k, v, do = _random_operands(rows, 4, 2, cosine=True)
    hs = torch.linspace(2.0, 18.0, 4)
    clean = sra_ref.window_attention(q, k, v, tok, off, 4, None, torch.float64, cosine_scale=hs, grad_o=do)
    idle = sra_ref.unreferenced_rows(tok, rows)
    for t in (q, k, v, do):
        t[idle] = float('nan')
    dirty = sra_ref.window_attention(q, k, v, tok, off, 4, None, torch.float64, cosine_scale=hs, grad_o=do)
    for name in clean:
        assert torch.equal(clean[name], dirty[name]), name
    assert clean['dscale'].shape == (64, 4)


@pytest.mark.parametrize('cap,copies', [(c, 1) for c in sra_ref.CAPS] + [(144, 8)])
def test_length_sweep_layout(cap, copies):
    sizes, tok, off, rows = sra_ref.length_sweep(cap, copies, 5)
    assert sorted(sizes.tolist()) == sorted(list(range(1, cap + 1)) * copies)
    m = cap * (cap + 1) // 2 * copies
    assert int(off[-1]) == m == len(tok) and rows == m + sra_ref.EXTRA_ROWS
    assert len(np.unique(tok)) == m and tok.min() >= 0 and tok.max() < rows
    idle = sra_ref.unreferenced_rows(tok, rows)
    assert len(idle) == sra_ref.EXTRA_ROWS and idle.min() < m // 2, 'unreferenced rows lie among the used ones'
    other = sra_ref.length_sweep(cap, copies, 6)[0]
    assert not np.array_equal(sizes, other)


@pytest.mark.parametrize('cosine', [False, True])
def test_one_hot_operands_route_exactly_at_every_length(cosine):
    """every length 1..144: the helper's own float64 gap assertion holds, all operands are bf16 numbers, and the float32
    restatement returns v[pi(i)] bit for bit"""
    heads = 4
    case = sra_ref.one_hot_case(np.arange(1, 145), heads, 7, cosine=cosine)
    for name in ('q', 'k', 'v'):
        assert torch.equal(case[name].to(torch.bfloat16).float(), case[name]), name
    got = sra_ref.window_attention(case['q'], case['k'], case['v'], case['tok'], case['off'], heads, case.get('scale'),
                                   torch.float32, cosine_scale=case.get('head_scale'))
    tok = torch.from_numpy(case['tok'].astype(np.int64))
    o = got['o'][tok].reshape(-1, heads, 16)
    want = torch.stack([case['v'][case['src'][:, h], h * 16:(h + 1) * 16] for h in range(heads)], 1)
    assert torch.equal(o, want)
    ms = case['max_score'].float()[None, :]
    assert float(((got['lse'][tok] - ms).abs() / ms).max()) <= 1e-6


def test_restatement_noise_of_the_four_sweeps(capsys):
    """the distance of the float32 restatement from float64 on the test's own operands: printed, and of the size the kernels'
    number format allows (a few 1e-6 on o at 144 tokens) - the GPU tests compute the same figure on their own operands"""
    for cosine in (False, True):
        for cap in sra_ref.CAPS:
            sizes, tok, off, rows = sra_ref.length_sweep(cap, 1, cap)
            q, k, v, do = _random_operands(rows, 8, cap, cosine=cosine)
            hs = 1.0 / (torch.rand(8, generator=torch.Generator().manual_seed(cap)) * 0.5 + 0.05) if cosine else None
            ref = sra_ref.window_attention(q, k, v, tok, off, 8, 0.25, torch.float64, cosine_scale=hs, grad_o=do)
            low = sra_ref.window_attention(q, k, v, tok, off, 8, 0.25, torch.float32, cosine_scale=hs, grad_o=do)
            noise = {n: float((low[n].double() - ref[n]).abs().max()) for n in ref}
            with capsys.disabled():
                print(f'\nrestatement noise cap {cap:3d} {"cosine" if cosine else "standard"}: '
                      + ' '.join(f'{n} {e:.2e}' for n, e in noise.items()))
            assert 0.0 < noise['o'] < 2e-5 and all(np.isfinite(e) for e in noise.values())
