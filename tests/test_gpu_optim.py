"""The training update on the GPU (csrc/optim.hip through sst_amd/optim.py): exact operands against closed forms, random data
against the float64 restatement of tests/optim_ref.py at a margin set by torch's own fp32 composition, alignment, repeatability,
skipped steps, absent gradients, the state's layout and a small training loop.

Shapes: one call holds tensors of numel 0, 1, 3, 7 x 5 (two-dimensional), 4097, one chunk + 1 and 3 chunks (empty, one element, a scalar tail only,
vector body + tail, more than one chunk, whole chunks); a second call holds 1500 one-element tensors (more chunks than the grid
cap of 1024 workgroups, so workgroups take several).  Two groups differ in lr and wd."""
import copy
import warnings

import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GROUPS = [dict(lr=1e-3, wd=0.05, b1=0.9, b2=0.999, eps=1e-8), dict(lr=2e-4, wd=0.0, b1=0.9, b2=0.999, eps=1e-8)]


def _chunk():
    from sst_amd import _lib
    return _lib.load().sst_optim_chunk_elems()


def _sizes(kind):
    """the shapes of a call's tensors"""
    if kind == 'mixed':
        c = _chunk()
        return [(0,), (1,), (3,), (7, 5), (4097,), (c + 1,), (3 * c,)]
    return [(1,)] * 1500


def _numel(shape):
    return int(np.prod(shape))


def _total(sizes):
    return sum(_numel(n) for n in sizes)


def _groups_of(sizes):
    return [i % 2 for i in range(len(sizes))]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class Ours(object):
    """a FusedAdamW over copies of the tensors of a problem, its state loaded in torch's layout where the problem has one"""

    def __init__(self, tensors, groups, params=None, **update_args):
        from sst_amd import optim
        self.tensors = tensors
        self.params = params or [torch.nn.Parameter(x['p'].detach().clone().to(DEV)) for x in tensors]
        pg = [[] for _ in groups]
        for p, x in zip(self.params, tensors):
            pg[x['group']].append(p)
        self.opt = optim.FusedAdamW([dict(params=ps, lr=h['lr'], weight_decay=h['wd'], betas=(h['b1'], h['b2']), eps=h['eps'])
                                     for ps, h in zip(pg, groups)])
        index = {id(p): i for i, p in enumerate(q for ps in pg for q in ps)}
        state = {index[id(p)]: {'step': torch.tensor(float(x['t'])), 'exp_avg': x['m'].clone(), 'exp_avg_sq': x['v'].clone()}
                 for p, x in zip(self.params, tensors) if x['t'] > 0}
        if state:
            sd = self.opt.state_dict()
            self.opt.load_state_dict({'state': state, 'param_groups': sd['param_groups']})
        self.update = optim.TrainingUpdate(self.opt, **update_args)
        self.set_grads([x['g'] for x in tensors])

    def set_grads(self, grads):
        for p, g in zip(self.params, grads):
            p.grad = None if g is None else g.detach().clone().to(DEV).view_as(p)

    def step(self):
        self.update.step()
        return self

    def result(self):
        """[(p, m, v)] of every tensor; zeros where a tensor has no state yet"""
        out = []
        for p in self.params:
            st = self.opt.state.get(p) or {}
            out.append((p.detach().clone(), st['exp_avg'].clone() if st else torch.zeros_like(p),
                        st['exp_avg_sq'].clone() if st else torch.zeros_like(p)))
        return out

    def steps(self):
        return [float(self.opt.state[p]['step']) if self.opt.state.get(p) else 0.0 for p in self.params]


def _check_margin(ours, torchs, want, what):
    """per tensor and quantity: gap(ours) <= max(4 gap(torch's fp32 composition), 1 fp32 ulp of the tensor's largest magnitude)"""
    worst, over = 0.0, []
    for i, (o, t, w) in enumerate(zip(ours, torchs, want)):
        for name, go, gt, ww in zip('pmv', R.gaps(o, w[:3]), R.gaps(t, w[:3]), w[:3]):
            bound = R.margin(gt, ww)
            worst = max(worst, go / bound)
            if go > bound:
                over.append(f'tensor {i} {name}: gap {go:.3e} > bound {bound:.3e} (torch gap {gt:.3e})')
    print(f'{what}: worst gap / bound = {worst:.3f}, {len(over)} of {3 * len(ours)} over the bound')
    assert not over, f'{what}: ' + '; '.join(over[:8])


# ----------------------------------------------------------------------------------------------------------------------
# exact operands
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['mixed', 'tiny'])
def test_decay_only_is_exact(kind):
    """g = 0, lr = 2^-4 (2^-3 in the second group), wd = 2^-2, p a multiple of 64: p * 63/64 (p * 31/32), m = v = 0"""
    sizes = _sizes(kind)
    groups = [dict(lr=2.0 ** -4, wd=2.0 ** -2, b1=0.9, b2=0.999, eps=1e-8), dict(lr=2.0 ** -3, wd=2.0 ** -2, b1=0.9, b2=0.999, eps=1e-8)]
    gen = torch.Generator().manual_seed(1)
    tensors = [dict(p=torch.randint(-1000, 1000, n, generator=gen).float() * 64, g=torch.zeros(n), m=torch.zeros(n),
                    v=torch.zeros(n), t=0, group=gi) for n, gi in zip(sizes, _groups_of(sizes))]
    run = Ours(tensors, groups).step()
    for x, (p, m, v) in zip(tensors, run.result()):
        want = x['p'] * (63 / 64 if x['group'] == 0 else 31 / 32)
        assert _same_bits(p.cpu(), want) and not m.any() and not v.any()
    assert run.steps() == [1.0] * len(sizes)
    assert float(run.update.grad_norm) == 0.0 and int(run.update.found_inf) == 0


@pytest.mark.parametrize('kind', ['mixed', 'tiny'])
def test_first_step_is_exact(kind):
    """b1 = 0.5, b2 = 0.75, eps = 0, wd = 0, g = +-2^k for k in -10..10: p - lr sign(g), m = g / 2, v = g^2 / 4"""
    sizes = _sizes(kind)
    groups = [dict(lr=2.0 ** -3, wd=0.0, b1=0.5, b2=0.75, eps=0.0), dict(lr=2.0 ** -2, wd=0.0, b1=0.5, b2=0.75, eps=0.0)]
    gen = torch.Generator().manual_seed(2)
    tensors = []
    for i, (n, gi) in enumerate(zip(sizes, _groups_of(sizes))):
        k = ((torch.arange(_numel(n)) + i) % 21 - 10).view(n)
        sign = torch.where((torch.arange(_numel(n)) + i) % 2 == 0, 1.0, -1.0).view(n)
        tensors.append(dict(p=torch.randint(-64, 64, n, generator=gen).float() / 8, g=sign * 2.0 ** k.float(),
                            m=torch.zeros(n), v=torch.zeros(n), t=0, group=gi))
    run = Ours(tensors, groups).step()
    for x, (p, m, v) in zip(tensors, run.result()):
        lr = groups[x['group']]['lr']
        assert _same_bits(p.cpu(), x['p'] - lr * torch.sign(x['g']))
        assert _same_bits(m.cpu(), x['g'] / 2) and _same_bits(v.cpu(), x['g'] * x['g'] / 4)


def test_norm_is_exact():
    """16 gradients of 4 over three tensors: total_norm == 16 exactly, clip_coef within one fp32 ulp of 8 / (16 + 1e-6)"""
    tensors = [dict(p=torch.zeros(n), g=torch.full((n,), 4.0), m=torch.zeros(n), v=torch.zeros(n), t=0, group=0) for n in (1, 3, 12)]
    run = Ours(tensors, GROUPS[:1], grad_clip=dict(max_norm=8, norm_type=2)).step()
    assert float(run.update.grad_norm) == 16.0
    want = 8 / (16 + 1e-6)
    assert abs(float(run.update.clip_coef) - want) <= R.ulp32(want)


# ----------------------------------------------------------------------------------------------------------------------
# random data
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['mixed', 'tiny'])
def test_one_step_from_a_state(kind):
    """step t = 7 from a given state, loss scale 32 and an active clip (max_norm 10; 5 for the small tensors' smaller norm)"""
    sizes = _sizes(kind)
    max_norm = 10.0 if kind == 'mixed' else 5.0
    tensors = R.random_problem(5, sizes, _groups_of(sizes), t=6, groups=GROUPS)
    want, norm, coef = R.update(tensors, GROUPS, max_norm=max_norm, scale=32.0)
    torchs, _ = R.torch_update(tensors, GROUPS, max_norm=max_norm, scale=32.0)
    run = Ours(tensors, GROUPS, grad_clip=dict(max_norm=max_norm, norm_type=2), loss_scale=32.0).step()
    n = _total(sizes)
    assert coef < 1.0 and abs(float(run.update.grad_norm) - norm) <= norm * n * 2.0 ** -52
    assert abs(float(run.update.clip_coef) - coef) <= R.ulp32(coef)
    assert run.steps() == [7.0] * len(sizes) and float(run.update.scale_tensor) == 32.0
    _check_margin(run.result(), torchs, want, f'one step ({kind})')


@pytest.mark.parametrize('kind', ['mixed', 'tiny'])
def test_one_step_is_correctly_rounded(kind):
    """every element of p, m and v is within half an fp32 ulp (of itself) of the float64 restatement, given the coefficient the
    device reports: the kernel evaluates an element in fp64 and rounds once.  2^-20 of slack for the float64 roundings."""
    sizes = _sizes(kind)
    max_norm = 10.0 if kind == 'mixed' else 5.0
    tensors = R.random_problem(5, sizes, _groups_of(sizes), t=6, groups=GROUPS)
    run = Ours(tensors, GROUPS, grad_clip=dict(max_norm=max_norm, norm_type=2), loss_scale=32.0).step()
    coef, inv = float(run.update.record.clip_coef64), float(run.update.record.inv_scale)
    assert inv == 1 / 32 and coef < 1.0 and float(run.update.clip_coef) == float(np.float32(coef))
    for x, got in zip(tensors, run.result()):
        h = GROUPS[x['group']]
        want = R.adamw(x['p'], x['g'], x['m'], x['v'], 7, h['lr'], h['wd'], h['b1'], h['b2'], h['eps'], inv, coef)
        for a, w in zip(got, want):
            half = 0.5 * np.spacing(np.abs(w).astype(np.float32)).astype(np.float64)
            assert np.all(np.abs(R.f64(a) - w) <= half * (1 + 2.0 ** -20))


def test_trajectory_of_five_steps():
    sizes = _sizes('mixed')
    gof = _groups_of(sizes)
    gen = torch.Generator().manual_seed(11)
    start = R.random_problem(6, sizes, gof)
    run = Ours(start, GROUPS, grad_clip=dict(max_norm=10, norm_type=2), loss_scale=32.0)
    want = [dict(x) for x in start]
    torchs = [dict(x) for x in start]
    for _ in range(5):
        grads = [torch.randn(n, generator=gen) * (10.0 if i % 3 == 0 else 0.1) for i, n in enumerate(sizes)]
        run.set_grads(grads)
        run.step()
        for x, y, g in zip(want, torchs, grads):
            x['g'] = y['g'] = g
        w, norm, _ = R.update(want, GROUPS, max_norm=10.0, scale=32.0)
        t, _ = R.torch_update(torchs, GROUPS, max_norm=10.0, scale=32.0)
        for x, (p, m, v, step) in zip(want, w):
            x.update(p=p, m=m, v=v, t=step)
        for y, (p, m, v) in zip(torchs, t):
            y.update(p=p, m=m, v=v, t=y['t'] + 1)
        assert abs(float(run.update.grad_norm) - norm) <= norm * _total(sizes) * 2.0 ** -52
    assert run.steps() == [5.0] * len(sizes)
    _check_margin(run.result(), [(y['p'], y['m'], y['v']) for y in torchs], [(x['p'], x['m'], x['v']) for x in want], 'five steps')


# ----------------------------------------------------------------------------------------------------------------------
# alignment and repeatability
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', [1, 2, 3])
def test_alignment_does_not_change_a_bit(offset):
    """the same values as 16-byte aligned tensors and as views at an odd element offset of a flat buffer, their gradients views
    of a world-1 GradBucketReducer: p, m, v, the norm and a second identical run agree bit for bit"""
    from sst_amd.parallel import GradBucketReducer
    sizes = [n for n in _sizes('mixed') if _numel(n)]
    tensors = R.random_problem(7, sizes, _groups_of(sizes), t=6, groups=GROUPS)
    args = dict(grad_clip=dict(max_norm=10, norm_type=2), loss_scale=32.0)
    aligned = Ours(tensors, GROUPS, **args).step()
    assert all(p.data_ptr() % 16 == 0 and p.grad.data_ptr() % 16 == 0 for p in aligned.params)
    again = Ours(tensors, GROUPS, **args).step()
    flat = torch.zeros(sum(_numel(n) + 4 for n in sizes) + 8, device=DEV)
    params, off = [], 0
    for x in tensors:
        n = x['p'].numel()
        start = (off + 3) // 4 * 4 + offset
        flat[start:start + n] = x['p'].to(DEV).view(-1)
        params.append(torch.nn.Parameter(flat[start:start + n].view_as(x['p'])))
        off = start + n
    assert all(p.data_ptr() % 16 == 4 * offset for p in params)
    views = Ours(tensors, GROUPS, params=params, **args)
    views.update.reducer = GradBucketReducer(params, n_buckets=2)
    views.step()
    assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(params, views.update.reducer.views))
    assert any(p.grad.data_ptr() % 16 for p in params)
    for a, b, c in zip(aligned.result(), again.result(), views.result()):
        for qa, qb, qc in zip(a, b, c):
            assert _same_bits(qa, qb) and _same_bits(qa, qc)
    assert _same_bits(aligned.update.record.buffer, again.update.record.buffer)
    assert _same_bits(aligned.update.record.buffer, views.update.record.buffer)


# ----------------------------------------------------------------------------------------------------------------------
# skipped steps and the loss scale
# ----------------------------------------------------------------------------------------------------------------------
def _poisoned(value, place):
    """one not-finite gradient element: the first element of the first tensor that moves with 16-byte accesses (thread 0 of the
    first chunk), the last element of a scalar tail behind such accesses (element 34 of the 7 x 5 tensor), the one-element
    tensor, the last element of the last tensor"""
    sizes = _sizes('mixed')
    tensors = R.random_problem(8, sizes, _groups_of(sizes), t=6, groups=GROUPS)
    where = {'first': (sizes.index((4097,)), 0), 'scalar_tail': (sizes.index((7, 5)), 34), 'one_element': (sizes.index((1,)), 0),
             'last': (len(sizes) - 1, _numel(sizes[-1]) - 1)}
    assert len(set(where.values())) == 4
    t, i = where[place]
    tensors[t]['g'].view(-1)[i] = value
    return tensors


@pytest.mark.parametrize('place', ['first', 'scalar_tail', 'one_element', 'last'])
@pytest.mark.parametrize('value', [float('inf'), float('nan')])
@pytest.mark.parametrize('loss_scale', [32.0, 'dynamic'])
def test_not_finite_gradient_skips_the_step(value, place, loss_scale):
    tensors = _poisoned(value, place)
    scale = dict(init_scale=1024.0, growth_interval=3) if loss_scale == 'dynamic' else loss_scale
    run = Ours(tensors, GROUPS, grad_clip=dict(max_norm=10, norm_type=2), loss_scale=scale)
    run.opt._ensure_state()
    before, steps = run.result(), run.steps()
    run.step()
    for a, b in zip(before, run.result()):
        assert all(_same_bits(x, y) for x, y in zip(a, b))
    assert run.steps() == steps == [6.0] * len(tensors)
    assert int(run.update.found_inf) == 1 and int(run.update.skipped_steps) == 1
    if loss_scale == 'dynamic':
        assert float(run.update.scale_tensor) == 512.0 and int(run.update.growth_tracker) == 0
    else:
        assert float(run.update.scale_tensor) == 32.0


def test_scale_grows_after_the_interval():
    sizes = [3, 35]
    tensors = R.random_problem(9, sizes, [0, 1])
    run = Ours(tensors, GROUPS, loss_scale=dict(init_scale=1024.0, growth_interval=3))
    seen = []
    for _ in range(4):
        run.step()
        seen.append((float(run.update.scale_tensor), int(run.update.growth_tracker)))
    assert seen == [(1024.0, 1), (1024.0, 2), (2048.0, 0), (2048.0, 1)]
    assert run.steps() == [4.0, 4.0] and int(run.update.skipped_steps) == 0
    loss = torch.ones((), device=DEV, requires_grad=True)
    assert float(run.update.scale(loss).detach()) == 2048.0


def test_nan_goes_through_without_a_loss_scale():
    """no loss scale and skip_nonfinite=False: the reference's plain hook; the NaN reaches p.  With skip_nonfinite=True it does not"""
    tensors = _poisoned(float('nan'), 'one_element')
    run = Ours(tensors, GROUPS, grad_clip=dict(max_norm=10, norm_type=2)).step()
    assert int(run.update.found_inf) == 1 and all(bool(torch.isnan(p).all()) for p, _, _ in run.result() if p.numel())
    assert run.steps() == [7.0] * len(tensors)
    run = Ours(tensors, GROUPS, grad_clip=dict(max_norm=10, norm_type=2), skip_nonfinite=True).step()
    assert run.steps() == [6.0] * len(tensors) and not any(bool(torch.isnan(p).any()) for p, _, _ in run.result())


# ----------------------------------------------------------------------------------------------------------------------
# presence, state
# ----------------------------------------------------------------------------------------------------------------------
def test_tensor_without_a_gradient_is_left_alone():
    sizes = [35, 4097, 3]
    tensors = R.random_problem(10, sizes, [0, 1, 0])
    grads = [x['g'] for x in tensors]
    tensors[1]['g'] = None
    run = Ours(tensors, GROUPS)
    p_before = run.params[1].detach().clone()
    run.step().step()
    assert run.steps() == [2.0, 0.0, 2.0] and run.params[1] not in run.opt.state
    assert _same_bits(run.params[1], p_before)
    assert not np.array_equal(R.f64(run.params[0]), R.f64(tensors[0]['p']))
    # its later first step is t = 1
    run.set_grads([None, grads[1], None])
    run.step()
    assert run.steps() == [2.0, 1.0, 2.0]
    alone = dict(tensors[1], g=grads[1])
    (wp, wm, wv, _), = R.update([alone], GROUPS)[0]
    (tp, tm, tv), = R.torch_update([alone], GROUPS)[0]
    _check_margin([run.result()[1]], [(tp, tm, tv)], [(wp, wm, wv)], 'late first step')


def _own_memory(a, b):
    """no tensor of optimizer a's state is a tensor of b's (torch's load_state_dict keeps what it is handed)"""
    mine = {t.data_ptr() for st in a.state.values() for t in st.values() if torch.is_tensor(t) and t.numel()}
    return not any(t.data_ptr() in mine for st in b.state.values() for t in st.values() if torch.is_tensor(t) and t.numel())


def _half_ulp(got, want, what):
    """every element of ours within half an fp32 ulp of itself of the float64 restatement (2^-20 of slack)"""
    for i, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip('pmv', g, w[:3]):
            half = 0.5 * np.spacing(np.abs(b).astype(np.float32)).astype(np.float64)
            assert np.all(np.abs(R.f64(a) - b) <= half * (1 + 2.0 ** -20)), f'{what}: tensor {i} {name}'


def test_state_dict_round_trip_with_torch():
    """state_dict() -> torch.optim.AdamW -> one further step of each; and back -> one further step: each optimizer on its own
    memory, ours within the margin of the restatement and, element by element, within half an ulp of it"""
    from sst_amd import optim
    sizes = [3, (7, 5), 4097]
    tensors = R.random_problem(12, sizes, [0, 1, 0])
    run = Ours(tensors, GROUPS).step().step()
    theirs_params = [torch.nn.Parameter(p.detach().clone()) for p in run.params]
    pg = [[theirs_params[0], theirs_params[2]], [theirs_params[1]]]
    theirs = torch.optim.AdamW([dict(params=ps) for ps in pg], lr=9.0)
    theirs.load_state_dict(run.opt.state_dict())          # a snapshot: copies of the counters and of the moments
    assert _own_memory(run.opt, theirs)
    assert [g['lr'] for g in theirs.param_groups] == [1e-3, 2e-4]
    assert all(float(theirs.state[p]['step']) == 2.0 for p in theirs_params)
    for p, q in zip(run.params, theirs_params):
        assert _same_bits(theirs.state[q]['exp_avg'], run.opt.state[p]['exp_avg'])
        assert _same_bits(theirs.state[q]['exp_avg_sq'], run.opt.state[p]['exp_avg_sq'])
    state = [dict(p=p.detach().clone(), g=torch.randn_like(p), m=run.opt.state[p]['exp_avg'].clone(),
                  v=run.opt.state[p]['exp_avg_sq'].clone(), t=2, group=x['group']) for p, x in zip(run.params, tensors)]
    want, _, _ = R.update(state, GROUPS)
    for p, q, x in zip(run.params, theirs_params, state):
        p.grad, q.grad = x['g'].clone(), x['g'].clone()
    run.step()
    theirs.step()
    assert run.steps() == [3.0] * 3 and all(float(theirs.state[q]['step']) == 3.0 for q in theirs_params)
    torchs = [(q.detach(), theirs.state[q]['exp_avg'], theirs.state[q]['exp_avg_sq']) for q in theirs_params]
    _check_margin(run.result(), torchs, want, 'after loading into torch')
    _half_ulp(run.result(), want, 'after loading into torch')
    # and back: a new FusedAdamW takes torch's state and steps like it
    back_params = [torch.nn.Parameter(q.detach().clone()) for q in theirs_params]
    back = optim.FusedAdamW([dict(params=[back_params[0], back_params[2]]), dict(params=[back_params[1]])], lr=9.0)
    back.load_state_dict(copy.deepcopy(theirs.state_dict()))       # torch's state_dict() holds its live tensors
    state = [dict(p=q.detach().clone(), g=torch.randn_like(q), m=theirs.state[q]['exp_avg'].clone(),
                  v=theirs.state[q]['exp_avg_sq'].clone(), t=3, group=x['group']) for q, x in zip(theirs_params, tensors)]
    want, _, _ = R.update(state, GROUPS)
    for p, q, x in zip(back_params, theirs_params, state):
        p.grad, q.grad = x['g'].clone(), x['g'].clone()
    back.step()
    theirs.step()
    assert _own_memory(back, theirs)
    ours = [(p.detach(), back.state[p]['exp_avg'], back.state[p]['exp_avg_sq']) for p in back_params]
    torchs = [(q.detach(), theirs.state[q]['exp_avg'], theirs.state[q]['exp_avg_sq']) for q in theirs_params]
    assert all(float(back.state[p]['step']) == 4.0 for p in back_params)
    assert all(float(theirs.state[q]['step']) == 4.0 for q in theirs_params)
    _check_margin(ours, torchs, want, 'after loading from torch')
    _half_ulp(ours, want, 'after loading from torch')


# ----------------------------------------------------------------------------------------------------------------------
# a training loop
# ----------------------------------------------------------------------------------------------------------------------
def _model():
    torch.manual_seed(3)
    m = torch.nn.Sequential()
    m.add_module('linear1', torch.nn.Linear(8, 16))
    m.add_module('norm', torch.nn.LayerNorm(16))
    m.add_module('linear2', torch.nn.Linear(16, 4))
    return m.to(DEV)


def test_training_loop_matches_torchs_composition():
    """3 steps of Linear - LayerNorm - Linear: fixed scale 32, clip 10, cyclic rate.  Ours and torch's composition (fp32, on the
    GPU) against the same loop in float64 with the restatement as its optimizer; no host synchronisation in our iteration and no
    device allocation in the steady-state update"""
    from sst_amd import optim
    cfg = dict(type='AdamW', lr=1e-3, betas=(0.9, 0.999), weight_decay=0.05, paramwise_cfg=dict(custom_keys={'norm': dict(decay_mult=0.)}))
    sched = dict(max_iters=10, target_ratio=(100, 1e-3), cyclic_times=1, step_ratio_up=0.4)
    ours_model = _model()
    torch_model = copy.deepcopy(ours_model)
    f64_model = copy.deepcopy(ours_model).double()
    x = torch.randn(32, 8, device=DEV)
    y = torch.randn(32, 4, device=DEV) * 30          # gradients large enough for the clip to bite

    def loss_of(model, xx, yy):
        return ((model(xx) - yy) ** 2).mean()

    opt = optim.build_optimizer(ours_model, cfg)
    update = optim.TrainingUpdate(opt, grad_clip=dict(max_norm=10, norm_type=2), loss_scale=32.0)
    lr = optim.CyclicLr(opt, **sched)
    allocs = []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('warn')        # (the mode's own notice that it is a prototype is not the step's)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        try:
            for it in range(3):
                lr.step(it)
                opt.zero_grad(set_to_none=True)
                update.scale(loss_of(ours_model, x, y)).backward()
                before = torch.cuda.memory_stats()['allocation.all.allocated']
                update.step()
                allocs.append(torch.cuda.memory_stats()['allocation.all.allocated'] - before)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    assert [str(w.message) for w in caught] == []
    assert allocs[1:] == [0, 0]
    assert float(update.clip_coef) < 1.0 and int(update.found_inf) == 0

    names = [n for n, _ in torch_model.named_parameters()]
    groups = [dict(lr=1e-3, wd=0.0 if 'norm' in n else 0.05, b1=0.9, b2=0.999, eps=1e-8) for n in names]
    topt = torch.optim.AdamW([dict(params=[p], lr=g['lr'], weight_decay=g['wd']) for p, g in zip(torch_model.parameters(), groups)])
    scaler = torch.amp.GradScaler('cuda', init_scale=32.0)
    f64_state = [dict(m=np.zeros(p.numel()), v=np.zeros(p.numel()), t=0) for p in f64_model.parameters()]
    for it in range(3):
        rate = R.cyclic(1e-3, it, **sched)
        for g in topt.param_groups:
            g['lr'] = rate
        topt.zero_grad(set_to_none=True)
        scaler.scale(loss_of(torch_model, x, y)).backward()
        scaler.unscale_(topt)
        torch.nn.utils.clip_grad_norm_(torch_model.parameters(), 10.0)
        scaler.step(topt)
        scaler.update(32.0)
        f64_model.zero_grad(set_to_none=True)
        (loss_of(f64_model, x.double(), y.double()) * 32.0).backward()
        tensors = [dict(p=p.detach().cpu().numpy().ravel(), g=p.grad.cpu().numpy().ravel(), m=s['m'], v=s['v'], t=s['t'], group=i)
                   for i, (p, s) in enumerate(zip(f64_model.parameters(), f64_state))]
        out, _, _ = R.update(tensors, [dict(g, lr=rate) for g in groups], max_norm=10.0, scale=32.0)
        with torch.no_grad():
            for p, s, (wp, wm, wv, t) in zip(f64_model.parameters(), f64_state, out):
                p.copy_(torch.from_numpy(wp).view_as(p))
                s.update(m=wm, v=wv, t=t)
    ours = [(p.detach().ravel(), opt.state[p]['exp_avg'].ravel(), opt.state[p]['exp_avg_sq'].ravel()) for p in ours_model.parameters()]
    torchs = [(p.detach().ravel(), topt.state[p]['exp_avg'].ravel(), topt.state[p]['exp_avg_sq'].ravel())
              for p in torch_model.parameters()]
    want = [(p.detach().cpu().numpy().ravel(), s['m'], s['v']) for p, s in zip(f64_model.parameters(), f64_state)]
    _check_margin(ours, torchs, want, 'training loop')
