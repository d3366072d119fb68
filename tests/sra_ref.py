"""Reference and operand recipes of the attention length sweeps (tests/test_gpu_sra_lengths.py, tests/test_sra_ref_host.py).
Plain torch, no GPU and no library needed to import.

window_attention   softmax(q k^T * scale) v per window and head (or the scaled cosine form), batched over windows padded
                   to the longest of a chunk, under autograd.  dtype=float64 is the reference; dtype=float32 is the
                   RESTATEMENT: the same formula in the kernels' own number format, whose distance from the reference is
                   the unit the GPU tests measure the kernels in.
length_sweep       every window length 1..cap, `copies` times each, shuffled, with a token list into a row set that has
                   EXTRA_ROWS rows no window refers to.
one_hot_case       operands for which the forward result is a pure gather: exact in fp32 and in bf16.
"""
import math

import numpy as np
import torch

CAPS = (64, 80, 112, 144)      # the largest window of each register-resident build (4, 5, 7 and 9 tiles of 16 tokens)
EXTRA_ROWS = 64                # rows of the operands that no window lists
LOG2E = 1.4426950408889634


def tiles(t):
    return (int(t) + 15) // 16


def token_list(sizes, rng):
    """-> (tok [M] int32, off [W + 1] int32, rows): tok is a permutation of M of the rows = M + EXTRA_ROWS row numbers, so the
    unreferenced rows lie scattered among the used ones"""
    m = int(np.sum(sizes))
    rows = m + EXTRA_ROWS
    tok = rng.permutation(rows)[:m].astype(np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return tok, off, rows


def length_sweep(cap, copies, seed):
    """-> (sizes [cap * copies], tok, off, rows): the window sizes 1..cap, each `copies` times, in a seeded shuffled order (the
    neighbours of a length differ between seeds)"""
    rng = np.random.default_rng(seed)
    sizes = np.repeat(np.arange(1, cap + 1, dtype=np.int64), copies)
    rng.shuffle(sizes)
    tok, off, rows = token_list(sizes, rng)
    return sizes, tok, off, rows


def unreferenced_rows(tok, rows):
    mask = np.ones(rows, dtype=bool)
    mask[tok] = False
    return np.nonzero(mask)[0]


def _chunks(sizes, chunk):
    """windows by ascending length in groups of `chunk`: little padding inside a group"""
    order = np.argsort(np.asarray(sizes), kind='stable')
    return [order[i:i + chunk] for i in range(0, len(order), chunk)]


def _gather_index(tok, off, wins, device):
    """-> (idx [W, T] long: row of window position p, the window's first row where p is past its end; mask [W, T])"""
    beg = torch.as_tensor(off[wins].astype(np.int64), device=device)
    length = torch.as_tensor((off[wins + 1] - off[wins]).astype(np.int64), device=device)
    p = torch.arange(int(length.max()), device=device)
    mask = p[None, :] < length[:, None]
    pos = beg[:, None] + torch.where(mask, p[None, :], torch.zeros_like(p)[None, :])
    return torch.as_tensor(tok.astype(np.int64), device=device)[pos], mask


def window_attention(q, k, v, tok, off, heads, scale, dtype, cosine_scale=None, grad_o=None, device=None, chunk=128):
    """q, k, v: [rows, heads * 16]; tok / off: numpy token list and window offsets.  Per window and head
    softmax(q k^T * scale) v, or with cosine_scale [heads]: softmax(normalize(q) normalize(k)^T * cosine_scale[h]) v.
    -> dict(o [rows, C], lse [rows, heads]) and, with grad_o, dq, dk, dv of sum(o * grad_o) by autograd and dscale
    [n_windows, heads]: every window's own share of d cosine_scale (their sum over windows is the gradient).
    Rows no window lists stay zero in every output and are never read (they may hold NaN)."""
    device = torch.device(device if device is not None else q.device)
    need_grad = grad_o is not None
    q, k, v = (t.detach().to(device=device, dtype=dtype).requires_grad_(need_grad) for t in (q, k, v))
    rows, c = q.shape
    hd = c // heads
    n_win = len(off) - 1
    sizes = np.asarray(off[1:] - off[:-1])
    cos = cosine_scale is not None
    if cos:   # one copy of the scale per window, so that autograd hands back every window's share
        sc_w = cosine_scale.detach().to(device=device, dtype=dtype)[None, :].repeat(n_win, 1).requires_grad_(need_grad)
    o = torch.zeros((rows, c), dtype=dtype, device=device)
    lse = torch.zeros((rows, heads), dtype=dtype, device=device)
    go = grad_o.detach().to(device=device, dtype=dtype) if need_grad else None
    for wins in _chunks(sizes, chunk):
        idx, mask = _gather_index(tok, off, wins, device)
        w, t = idx.shape
        qw, kw, vw = (x[idx].reshape(w, t, heads, hd).permute(0, 2, 1, 3) for x in (q, k, v))     # [W, H, T, 16]
        if cos:
            qw = torch.nn.functional.normalize(qw, dim=-1)
            kw = torch.nn.functional.normalize(kw, dim=-1)
            s = torch.matmul(qw, kw.transpose(-1, -2)) * sc_w[torch.as_tensor(wins, device=device)][:, :, None, None]
        else:
            s = torch.matmul(qw, kw.transpose(-1, -2)) * scale
        s = s.masked_fill(~mask[:, None, None, :], -math.inf)
        l = torch.logsumexp(s, dim=-1)                                                            # [W, H, T]
        ow = torch.matmul(torch.softmax(s, dim=-1), vw).permute(0, 2, 1, 3).reshape(w, t, c)
        o[idx[mask]] = ow[mask].detach()
        lse[idx[mask]] = l.permute(0, 2, 1)[mask].detach()
        if need_grad:
            (ow[mask] * go[idx[mask]]).sum().backward()
    out = dict(o=o, lse=lse)
    if need_grad:
        out.update(dq=q.grad, dk=k.grad, dv=v.grad)
        if cos:
            out['dscale'] = sc_w.grad
    return out


def _codes_to_rows(codes):
    """[..] integer codes below 2^16 -> [.., 16] float32 of +-1 (bit b set: +1)"""
    bits = (codes[..., None] >> np.arange(16)) & 1
    return (2 * bits - 1).astype(np.float32)


def one_hot_case(sizes, heads, seed, cosine=False):
    """Operands whose attention output is a pure gather.  In every window and head, key row j is the +-1 vector of a 16-bit code
    distinct within the window (one code per head), query i is 256 * key pi(i) for a seeded map pi of the window into itself
    (a permutation in even windows, a map with repeats in odd ones; one map per head), v holds integers in [-8, 8].  With the
    scale 0.25 the winning score is 1024 and every other at most 896: 128 * log2(e) = 184 below the row maximum in the log2
    domain, so its weight is exactly 0 in fp32, the winner's is exp2(0) = 1, the row sum 1 and o[i] == v[pi(i)] bit for bit.
    cosine=True: q and k rows carry per-row powers of two in addition (the normalisation removes them) and the case is meant for
    head_scale >= 1024: the cosine of distinct codes is at most 0.875, the gap again >= 128 * log2(e).
    The gap (>= 160) and the routing are asserted here in float64 before anything is returned.
    -> dict(q, k, v [rows, C] float32; tok, off, rows; src [M, heads] int64: the row whose v the query at token-list position p
    receives in head h; max_score [heads] float64; scale or head_scale)"""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    tok, off, rows = token_list(sizes, rng)
    m, c = int(off[-1]), heads * 16
    codes = np.zeros((m, heads), dtype=np.int64)
    src_pos = np.zeros((m, heads), dtype=np.int64)          # token-list position of the key a query selects
    for w, t in enumerate(sizes):
        b = int(off[w])
        for h in range(heads):
            codes[b:b + t, h] = rng.choice(1 << 16, size=int(t), replace=False)
            src_pos[b:b + t, h] = b + (rng.permutation(int(t)) if w % 2 == 0 else rng.integers(0, int(t), size=int(t)))
    krow = _codes_to_rows(codes).reshape(m, c)
    qrow = 256.0 * _codes_to_rows(codes[src_pos, np.arange(heads)[None, :]]).reshape(m, c)
    if cosine:   # powers of two per row: removed exactly by the normalisation (the norm is 4 * 2^e)
        krow = krow * np.exp2(rng.integers(-3, 4, size=(m, 1))).astype(np.float32)
        qrow = qrow * np.exp2(rng.integers(-3, 4, size=(m, 1))).astype(np.float32)
    q = np.zeros((rows, c), dtype=np.float32)
    k = np.zeros((rows, c), dtype=np.float32)
    v = np.zeros((rows, c), dtype=np.float32)
    q[tok], k[tok] = qrow, krow
    v[tok] = rng.integers(-8, 9, size=(m, c)).astype(np.float32)
    head_scale = (1024.0 * (1.0 + 0.5 * (np.arange(heads) % 3))) if cosine else None
    case = dict(q=torch.from_numpy(q), k=torch.from_numpy(k), v=torch.from_numpy(v), tok=tok, off=off, rows=rows,
                src=torch.from_numpy(tok.astype(np.int64)[src_pos]), sizes=sizes)
    if cosine:
        case['head_scale'] = torch.from_numpy(head_scale.astype(np.float32))
        case['max_score'] = torch.from_numpy(head_scale.astype(np.float64))
    else:
        case['scale'] = 0.25
        case['max_score'] = torch.full((heads,), 1024.0, dtype=torch.float64)
    _assert_one_hot_gap(case, heads, src_pos)
    return case


def _assert_one_hot_gap(case, heads, src_pos, min_gap=160.0):
    """float64: in every row the score of key pi(i) is the maximum, equals max_score, and every other score of the window lies
    at least min_gap below it in the log2 domain"""
    tok, off = case['tok'], case['off']
    q, k = case['q'].double(), case['k'].double()
    sizes = np.asarray(off[1:] - off[:-1])
    for wins in _chunks(sizes, 128):
        idx, mask = _gather_index(tok, off, wins, 'cpu')
        w, t = idx.shape
        qw, kw = (x[idx].reshape(w, t, heads, 16).permute(0, 2, 1, 3) for x in (q, k))
        if 'head_scale' in case:
            qw, kw = torch.nn.functional.normalize(qw, dim=-1), torch.nn.functional.normalize(kw, dim=-1)
            s = torch.matmul(qw, kw.transpose(-1, -2)) * case['head_scale'].double()[None, :, None, None]
        else:
            s = torch.matmul(qw, kw.transpose(-1, -2)) * case['scale']
        s = s.masked_fill(~mask[:, None, None, :], -math.inf) * LOG2E
        top = s.topk(min(2, t), dim=-1)
        beg = torch.as_tensor(off[wins].astype(np.int64))
        want = torch.as_tensor(src_pos)[(beg[:, None] + torch.arange(t)[None, :]).clamp(max=len(src_pos) - 1)] - beg[:, None, None]
        want = want.permute(0, 2, 1)                                                               # [W, H, T]
        valid = mask[:, None, :].expand(w, heads, t)
        assert bool((top.indices[..., 0] == want)[valid].all()), 'one_hot_case: the winning key is not pi(i)'
        ms = case['max_score'][None, :, None] * LOG2E
        assert float((top.values[..., 0] - ms).abs()[valid].max()) <= 1e-9 * float(ms.max()), 'one_hot_case: max score'
        if t > 1:
            gap = (top.values[..., 0] - top.values[..., 1])[valid]
            assert float(gap.min()) >= min_gap, f'one_hot_case: gap {float(gap.min())} < {min_gap}'
