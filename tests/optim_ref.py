"""The float64 restatement of the training update (sst_amd/optim.py, csrc/optim.hip) and of its schedules, with the torch
composition it stands for (GradScaler.unscale_ + clip_grad_norm_ + AdamW.step + GradScaler.update) as a second, fp32, witness.

Everything here is plain numpy / Python float64 on the fp32 inputs: no rounding to fp32 anywhere.  The loss scales the tests use
are powers of two, so ``g * inv_scale`` is exact in either precision."""
import math

import numpy as np
import torch


def ulp32(x):
    """one fp32 unit in the last place at magnitude |x| (the smallest normal's for 0)"""
    return float(np.spacing(np.float32(max(abs(float(x)), float(np.finfo(np.float32).tiny)))))


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)


def total_norm(grads, inv_scale=1.0):
    """sqrt of the exactly rounded sum of (g * inv_scale)^2 over all gradients"""
    return math.sqrt(math.fsum(float(x) for g in grads for x in (f64(g).ravel() * inv_scale) ** 2))


def clip_coef(norm, max_norm):
    return 1.0 if max_norm is None else min(1.0, max_norm / (norm + 1e-6))


def adamw(p, g, m, v, t, lr, wd, b1, b2, eps, inv_scale=1.0, coef=1.0):
    """one AdamW step number ``t`` (>= 1) of one tensor; returns float64 (p, m, v)"""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    g = g * inv_scale * coef
    p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - (lr / (1 - b1 ** t)) * m / (np.sqrt(v) / math.sqrt(1 - b2 ** t) + eps)
    return p, m, v


def scaler_update(scale, tracker, found_inf, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
    """torch.amp.GradScaler.update: (scale, growth_tracker) after a step"""
    if found_inf:
        return scale * backoff_factor, 0
    tracker += 1
    if tracker == growth_interval:
        return scale * growth_factor, 0
    return scale, tracker


def update(tensors, groups, max_norm=None, scale=1.0):
    """the whole update of one step.  tensors: dicts with p, g (None = no gradient), m, v, t (steps done so far), group;
    groups: dicts with lr, wd, b1, b2, eps.  Returns ([(p, m, v, t)], total_norm, clip_coef) in float64; a tensor without a
    gradient comes back unchanged."""
    inv = 1.0 / scale
    norm = total_norm([x['g'] for x in tensors if x['g'] is not None], inv)
    coef = clip_coef(norm, max_norm)
    out = []
    for x in tensors:
        if x['g'] is None:
            out.append((f64(x['p']), f64(x['m']), f64(x['v']), x['t']))
            continue
        h = groups[x['group']]
        p, m, v = adamw(x['p'], x['g'], x['m'], x['v'], x['t'] + 1, h['lr'], h['wd'], h['b1'], h['b2'], h['eps'], inv, coef)
        out.append((p, m, v, x['t'] + 1))
    return out, norm, coef


def torch_update(tensors, groups, max_norm=None, scale=None, device='cpu', optimizer_kwargs=None):
    """the same step by torch in fp32 on ``device``: GradScaler (when ``scale``) + clip_grad_norm_ + torch.optim.AdamW.
    Returns ([(p, m, v)] as fp32 tensors, total_norm tensor or None)."""
    params, pg = [], [[] for _ in groups]
    for x in tensors:
        p = torch.nn.Parameter(x['p'].detach().clone().to(device))
        p.grad = None if x['g'] is None else x['g'].detach().clone().to(device)
        params.append(p)
        pg[x['group']].append(p)
    opt = torch.optim.AdamW([dict(params=ps, lr=h['lr'], weight_decay=h['wd'], betas=(h['b1'], h['b2']), eps=h['eps'])
                             for ps, h in zip(pg, groups) if ps], **(optimizer_kwargs or {}))
    for p, x in zip(params, tensors):
        if x['t'] > 0:
            opt.state[p] = {'step': torch.tensor(float(x['t'])), 'exp_avg': x['m'].detach().clone().to(device),
                            'exp_avg_sq': x['v'].detach().clone().to(device)}
    scaler = None
    if scale is not None:
        scaler = torch.amp.GradScaler(torch.device(device).type, init_scale=float(scale), growth_interval=10 ** 9)
        scaler.scale(torch.zeros(1, device=device))     # the scaler makes its device tensors on first use
        scaler.unscale_(opt)
    norm = None
    if max_norm is not None:
        norm = torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], max_norm)
    if scaler is not None:
        scaler.step(opt)
        scaler.update()
    else:
        opt.step()
    out = []
    for p, x in zip(params, tensors):
        st = opt.state.get(p, {})
        out.append((p.detach(), st.get('exp_avg', x['m']), st.get('exp_avg_sq', x['v'])))
    return out, norm


def gaps(got, want):
    """max-abs gap per quantity (p, m, v) between fp32 tensors ``got`` and the float64 arrays ``want``"""
    return [float(np.max(np.abs(f64(a) - b))) if b.size else 0.0 for a, b in zip(got, want)]


def margin(torch_gap, want):
    """the bound of the GPU tests: 4 x the gap of torch's own fp32 composition, at least one fp32 ulp of the tensor's largest
    magnitude"""
    return max(4.0 * torch_gap, ulp32(np.max(np.abs(want)) if want.size else 0.0))


# ----------------------------------------------------------------------------------------------------------------------
# schedules (mmcv 1.3.9: runner/hooks/lr_updater.py, momentum_updater.py; restated from their documented formulas)
# ----------------------------------------------------------------------------------------------------------------------
def anneal(a, b, f):
    return b + 0.5 * (a - b) * (math.cos(math.pi * f) + 1)


def cyclic(base, it, max_iters, target_ratio, cyclic_times=1, step_ratio_up=0.4):
    per = max_iters // cyclic_times
    up = int(step_ratio_up * per)
    it %= per
    if it < up:
        return anneal(base, base * target_ratio[0], it / up)
    return anneal(base * target_ratio[0], base * target_ratio[1], (it - up) / (per - up))


def random_problem(seed, numels, groups_of=None, t=0, groups=None, device='cpu'):
    """tensors of these sizes (an element count or a shape each) with random p and g.  For t > 0 the state is what t float64 steps on random gradients of the same
    spread leave behind, rounded to fp32: m and v of the size a training run has at that point"""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(numels):
        spread = 10.0 if i % 3 == 0 else 0.1
        group = 0 if groups_of is None else groups_of[i]
        n = tuple(n) if isinstance(n, (tuple, list)) else (n,)
        p, m, v = f64(torch.randn(n, generator=gen)), np.zeros(n), np.zeros(n)
        for k in range(t):
            h = groups[group]
            g = torch.randn(n, generator=gen) * spread
            p, m, v = adamw(p, g, m, v, k + 1, h['lr'], h['wd'], h['b1'], h['b2'], h['eps'])
        g = torch.randn(n, generator=gen) * spread
        p, m, v = (torch.from_numpy(np.asarray(a)).float() for a in (p, m, v))
        out.append(dict(p=p.to(device), g=g.to(device), m=m.to(device), v=v.to(device), t=t, group=group))
    return out
