"""The host side of the training update (sst_amd/optim.py): the float64 restatement of tests/optim_ref.py against torch's own
composition on the CPU, the schedules, the parameter groups, the config reading and every refusal.  No kernel runs."""
import ast
import math
import os

import numpy as np
import pytest
import torch

import optim_ref as R
from conftest import GOLDEN
from sst_amd import optim
from test_configs_build import REF

REF_CONFIGS = os.path.join(REF, 'configs')
TRAIN = os.path.join(GOLDEN, 'configs', 'train')
# cosine_2x.py at its peak rate with and without the decay of its 'norm' key
GROUPS = [dict(lr=1e-3, wd=0.05, b1=0.9, b2=0.999, eps=1e-8), dict(lr=2e-4, wd=0.0, b1=0.9, b2=0.999, eps=1e-8)]
NUMELS = [1, 3, 35, 4097, 130]


def _train_settings(name):
    return ast.literal_eval(open(os.path.join(TRAIN, name + '.train.py')).read())


@pytest.mark.parametrize('t,seed', [(6, 9), (6, 10), (2, 11)])
def test_restatement_is_torchs_composition(t, seed):
    """GradScaler('cpu').unscale_ + clip_grad_norm_ + torch.optim.AdamW on CPU tensors is what the restatement describes: per
    tensor and quantity the gap is at most one fp32 ulp of the tensor's largest value.  That holds while the clip does not bite
    (max_norm 35 here): torch forms the norm in fp32, pairwise, so its norm of N numbers - and with it an active coefficient,
    and through it every gradient - is only within (log2 N + 4) 2^-24 of the exact one, which the second half checks.  The step
    starts from a state (as the GPU test's does): a first step's v = fp32(1 - b2) g g is three fp32 roundings, up to 1.5 ulp
    of itself, so one ulp is no bound there; test_restatement_exact_cases pins the first step instead."""
    tensors = R.random_problem(seed, NUMELS, [0, 1, 0, 1, 0], t=t, groups=GROUPS)
    want, norm, coef = R.update(tensors, GROUPS, max_norm=35.0, scale=32.0)
    got, torch_norm = R.torch_update(tensors, GROUPS, max_norm=35.0, scale=32.0)
    norm_bound = (math.log2(sum(NUMELS)) + 4) * 2.0 ** -24
    assert coef == 1.0 and abs(float(torch_norm) - norm) <= norm * norm_bound
    for (p, m, v), (wp, wm, wv, _) in zip(got, want):
        for gap, w in zip(R.gaps((p, m, v), (wp, wm, wv)), (wp, wm, wv)):
            assert gap <= R.ulp32(np.max(np.abs(w)))
    # an active clip: the gradients torch leaves behind are g * inv_scale * coef with its own fp32 coefficient
    want, norm, coef = R.update(tensors, GROUPS, max_norm=10.0, scale=32.0)
    params = [torch.nn.Parameter(x['p'].clone()) for x in tensors]
    for p, x in zip(params, tensors):
        p.grad = x['g'] / 32.0
    torch_norm = torch.nn.utils.clip_grad_norm_(params, 10.0)
    assert coef < 1.0 and abs(float(torch_norm) - norm) <= norm * norm_bound
    for p, x in zip(params, tensors):
        exact = R.f64(x['g']) / 32.0 * coef
        assert np.all(np.abs(R.f64(p.grad) - exact) <= np.abs(exact) * (norm_bound + 3 * 2.0 ** -24))


def test_restatement_exact_cases():
    """the closed forms the GPU test pins, in the restatement and in torch on the CPU"""
    h = [dict(lr=2.0 ** -4, wd=2.0 ** -2, b1=0.9, b2=0.999, eps=1e-8)]
    p = torch.arange(-8, 8, dtype=torch.float32) * 64
    x = [dict(p=p, g=torch.zeros(16), m=torch.zeros(16), v=torch.zeros(16), t=0, group=0)]
    (wp, _, _, _), = R.update(x, h)[0]
    (tp, _, _), = R.torch_update(x, h)[0]
    assert np.array_equal(wp, R.f64(p) * 63 / 64) and np.array_equal(R.f64(tp), wp)
    h = [dict(lr=2.0 ** -3, wd=0.0, b1=0.5, b2=0.75, eps=0.0)]
    k = torch.arange(-10, 11, dtype=torch.float32)
    g = torch.cat([2.0 ** k, -(2.0 ** k)])
    p = torch.linspace(-3, 3, g.numel())
    x = [dict(p=p, g=g, m=torch.zeros_like(g), v=torch.zeros_like(g), t=0, group=0)]
    (wp, wm, wv, _), = R.update(x, h)[0]
    (tp, tm, tv), = R.torch_update(x, h)[0]
    assert np.array_equal(wp, R.f64(p) - 2.0 ** -3 * np.sign(R.f64(g)))
    assert np.array_equal(wm, R.f64(g) / 2) and np.array_equal(wv, R.f64(g) ** 2 / 4)
    assert np.array_equal(R.f64(tp), R.f64((p.double() - 2.0 ** -3 * torch.sign(g).double()).float()))
    assert np.array_equal(R.f64(tm), wm) and np.array_equal(R.f64(tv), wv)
    grads = [torch.full((n,), 4.0) for n in (1, 3, 12)]
    assert R.total_norm(grads) == 16.0 and R.clip_coef(16.0, 8.0) == 8 / (16 + 1e-6)


def test_scaler_restatement_is_gradscalers():
    s = torch.amp.GradScaler('cpu', init_scale=1024.0, growth_interval=3)
    p = torch.nn.Parameter(torch.zeros(2))
    opt = torch.optim.SGD([p], lr=0.1)
    s.scale(torch.zeros(1))
    scale, tracker = 1024.0, 0
    for bad in (False, False, True, False, False, False, False):
        p.grad = torch.tensor([float('inf') if bad else 1.0, 0.0])
        s.unscale_(opt)
        s.step(opt)
        s.update()
        scale, tracker = R.scaler_update(scale, tracker, bad, growth_interval=3)
        assert s.get_scale() == scale and s._get_growth_tracker() == tracker


SCHEDULES = {   # the two shipped schedules: cosine_2x.py, cyclic_20e.py
    'cosine_2x': dict(base=1e-5, target_ratio=(100, 1e-3), step_ratio_up=0.1),
    'cyclic_20e': dict(base=1e-4, target_ratio=(10, 1e-4), step_ratio_up=0.4),
    'cyclic_20e_momentum': dict(base=0.9, target_ratio=(0.85 / 0.95, 1), step_ratio_up=0.4),
}


@pytest.mark.parametrize('name', sorted(SCHEDULES))
@pytest.mark.parametrize('max_iters,cyclic_times', [(1000, 1), (1003, 2)])
def test_cyclic_schedules(name, max_iters, cyclic_times):
    s = SCHEDULES[name]
    momentum = name.endswith('momentum')
    p = torch.nn.Parameter(torch.zeros(3))
    opt = optim.FusedAdamW([p], lr=1e-4 if momentum else s['base'], betas=(s['base'] if momentum else 0.9, 0.999))
    cls = optim.CyclicMomentum if momentum else optim.CyclicLr
    sched = cls(opt, max_iters, s['target_ratio'], cyclic_times=cyclic_times, step_ratio_up=s['step_ratio_up'])
    per = max_iters // cyclic_times
    up = int(s['step_ratio_up'] * per)
    r0, r1 = s['target_ratio']
    for it in (0, up - 1, up, per - 1, per):
        sched.step(it)
        got = opt.param_groups[0]['betas'][0] if momentum else opt.param_groups[0]['lr']
        assert got == pytest.approx(R.cyclic(s['base'], it, max_iters, s['target_ratio'], cyclic_times, s['step_ratio_up']),
                                    rel=1e-15)
        if momentum:
            assert opt.param_groups[0]['betas'][1] == 0.999 and opt.param_groups[0]['lr'] == 1e-4
    # the shape of the cycle: base at 0 and again at `per`, the peak at `up`, close to the final ratio at the end
    assert R.cyclic(s['base'], 0, max_iters, s['target_ratio'], cyclic_times, s['step_ratio_up']) == pytest.approx(s['base'])
    assert R.cyclic(s['base'], up, max_iters, s['target_ratio'], cyclic_times, s['step_ratio_up']) == pytest.approx(s['base'] * r0)
    assert R.cyclic(s['base'], per, max_iters, s['target_ratio'], cyclic_times, s['step_ratio_up']) == pytest.approx(s['base'])
    last = R.cyclic(s['base'], per - 1, max_iters, s['target_ratio'], cyclic_times, s['step_ratio_up'])
    assert abs(last - s['base'] * r1) <= abs(s['base'] * (r0 - r1)) * (math.pi / (per - up)) ** 2


class _Block(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.linear1 = torch.nn.Linear(4, 6)
        self.norm1 = torch.nn.LayerNorm(6)
        self.linear2 = torch.nn.Linear(6, 2)
        self.pre_norm_proj = torch.nn.Linear(2, 2, bias=False)     # 'norm' in the name of a layer that is not a norm
        self.frozen = torch.nn.Parameter(torch.zeros(3), requires_grad=False)


def test_custom_keys_groups():
    model = _Block()
    opt = optim.build_optimizer(model, dict(type='AdamW', lr=1e-5, betas=(0.9, 0.999), weight_decay=0.05,
                                            paramwise_cfg=dict(custom_keys={'norm': dict(decay_mult=0.)})))
    by_wd = {g['weight_decay']: g for g in opt.param_groups}
    assert sorted(by_wd) == [0.0, 0.05] and all(g['lr'] == 1e-5 and g['betas'] == (0.9, 0.999) for g in opt.param_groups)
    names = {id(p): n for n, p in model.named_parameters()}
    assert sorted(names[id(p)] for p in by_wd[0.0]['params']) == ['norm1.bias', 'norm1.weight', 'pre_norm_proj.weight']
    assert sorted(names[id(p)] for p in by_wd[0.05]['params']) == ['linear1.bias', 'linear1.weight', 'linear2.bias',
                                                                  'linear2.weight']
    # the longest key wins, then the alphabetical order; lr_mult scales the rate
    opt = optim.build_optimizer(model, dict(type='AdamW', lr=1.0, weight_decay=1.0, paramwise_cfg=dict(custom_keys={
        'norm': dict(decay_mult=0.), 'pre_norm': dict(lr_mult=0.5), 'linear1': dict(lr_mult=0.1, decay_mult=2.)})))
    got = {names[id(p)]: (g['lr'], g['weight_decay']) for g in opt.param_groups for p in g['params']}
    assert got == {'linear1.weight': (0.1, 2.0), 'linear1.bias': (0.1, 2.0), 'norm1.weight': (1.0, 0.0), 'norm1.bias': (1.0, 0.0),
                   'linear2.weight': (1.0, 1.0), 'linear2.bias': (1.0, 1.0), 'pre_norm_proj.weight': (0.5, 1.0)}


@pytest.mark.parametrize('sub,name', [('sst_refactor', 'sst_waymoD5_1x_3class_8heads_v2'), ('fsdv2', 'fsdv2_nusc_1x')])
def test_build_training_update_on_shipped_configs(sub, name):
    """the training settings of two shipped configs (stored resolved under tests/golden/configs/train; compared with the config
    text where the reference tree is present, and then also built from that text)"""
    settings = _train_settings(name)
    sources = [settings]
    path = os.path.join(REF_CONFIGS, sub, name + '.py')
    if os.path.exists(path):
        text = open(path).read()
        resolved = optim.resolve_config(text, os.path.dirname(path))
        assert {k: resolved.get(k) for k in settings} == settings
        sources.append(text)
    for cfg in sources:
        model = _Block()
        update, schedules = optim.build_training_update(model, cfg, max_iters=1000, base_dir=os.path.dirname(path))
        opt = update.optimizer
        if name.startswith('sst'):
            assert update.max_norm == 10.0 and update.scale_mode == optim.SCALE_FIXED and update.init_scale == 32.0
            assert update.skip_nonfinite
            assert sorted((g['lr'], g['weight_decay']) for g in opt.param_groups) == [(1e-5, 0.0), (1e-5, 0.05)]
            assert [type(s) for s in schedules] == [optim.CyclicLr]
            schedules[0].step(100)
            assert all(g['lr'] == pytest.approx(1e-3) for g in opt.param_groups)
        else:
            assert update.max_norm == 35.0 and update.scale_mode == optim.SCALE_NONE and not update.skip_nonfinite
            assert [(g['lr'], g['weight_decay'], g['betas']) for g in opt.param_groups] == [(2e-4, 0.01, (0.9, 0.999))]
            assert [type(s) for s in schedules] == [optim.CyclicLr, optim.CyclicMomentum]
            for s in schedules:
                s.step(400)
            assert opt.param_groups[0]['lr'] == pytest.approx(2e-3)
            assert opt.param_groups[0]['betas'] == (pytest.approx(0.9 * 0.85 / 0.95), 0.999)


def test_config_text_with_base_files(tmp_path):
    (tmp_path / 'base').mkdir()
    (tmp_path / 'base' / 'schedule.py').write_text(
        "optimizer = dict(type='AdamW', lr=1e-3, weight_decay=0.1)\noptimizer_config = dict(grad_clip=dict(max_norm=5, norm_type=2))\n"
        "lr_config = dict(policy='cyclic', target_ratio=(10, 1e-4), cyclic_times=1, step_ratio_up=0.4)\nmomentum_config = None\n")
    text = "_base_ = ['base/schedule.py']\noptimizer = dict(lr=2e-3)\nfp16 = dict(loss_scale='dynamic')\n"
    update, schedules = optim.build_training_update(_Block(), text, 50, base_dir=str(tmp_path))
    assert update.optimizer.param_groups[0]['lr'] == 2e-3 and update.optimizer.param_groups[0]['weight_decay'] == 0.1
    assert update.max_norm == 5.0 and update.scale_mode == optim.SCALE_DYNAMIC and update.init_scale == 2.0 ** 16
    assert len(schedules) == 1
    with pytest.raises(ValueError, match='base_dir'):
        optim.build_training_update(_Block(), text, 50)


def test_state_dict_has_torchs_layout():
    """the state_dict of a FusedAdamW loads into torch.optim.AdamW and back (CPU: no step is taken)"""
    ps = [torch.nn.Parameter(torch.randn(n)) for n in (3, 5)]
    theirs = torch.optim.AdamW(ps, lr=1e-3, betas=(0.8, 0.9), eps=1e-6, weight_decay=0.02)
    for p in ps:
        p.grad = torch.randn_like(p)
    theirs.step()
    ours = optim.FusedAdamW(ps, lr=1.0)
    ours.load_state_dict(theirs.state_dict())
    sd = ours.state_dict()
    assert sd['param_groups'][0]['lr'] == 1e-3 and sd['param_groups'][0]['betas'] == (0.8, 0.9)
    assert sorted(sd['state']) == [0, 1] and sorted(sd['state'][0]) == ['exp_avg', 'exp_avg_sq', 'step']
    again = torch.optim.AdamW(ps, lr=5.0)
    again.load_state_dict(sd)
    for p in ps:
        assert float(again.state[p]['step']) == 1.0
        assert torch.equal(again.state[p]['exp_avg'], theirs.state[p]['exp_avg'])
        assert torch.equal(again.state[p]['exp_avg_sq'], theirs.state[p]['exp_avg_sq'])
    again.step()                     # torch accepts the groups as they came back
    ours.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in ps)


def test_chunk_table_covers_every_tensor_once():
    chunk = 4096
    numels = [0, 1, 3, 35, 4097, chunk, chunk + 1, 3 * chunk, 0, 2]
    table = optim.chunk_table(numels, chunk)
    for i, n in enumerate(numels):
        rows = table[table['tensor'] == i]
        assert list(rows['start']) == list(range(0, n, chunk))
        assert int(rows['count'].sum()) == n and all(0 < c <= chunk for c in rows['count'])
        assert all(int(s) + int(c) <= n for s, c in zip(rows['start'], rows['count']))
    assert len(optim.chunk_table([], chunk)) == 0 and len(optim.chunk_table([0, 0], chunk)) == 0
    assert optim._TENSOR_DTYPE.itemsize == 48 and optim._CHUNK_DTYPE.itemsize == 16


def test_refusals():
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match='amsgrad'):
        optim.FusedAdamW([p], amsgrad=True)
    with pytest.raises(ValueError, match='maximize'):
        optim.FusedAdamW([p], maximize=True)
    with pytest.raises(ValueError, match='amsgrad'):
        optim.FusedAdamW([dict(params=[p], amsgrad=True)])
    with pytest.raises(TypeError, match='non-fp32'):
        optim.FusedAdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(TypeError, match='non-fp32'):
        optim.FusedAdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))])
    with pytest.raises(ValueError, match='non-contiguous'):
        optim.FusedAdamW([torch.nn.Parameter(torch.zeros(4, 6).t())])
    with pytest.raises(ValueError, match='several devices'):
        optim.FusedAdamW([p, torch.nn.Parameter(torch.zeros(4, device='meta'))])
    many = [dict(params=[torch.nn.Parameter(torch.zeros(2))], lr=1e-3 * (i + 1)) for i in range(9)]
    with pytest.raises(ValueError, match='more than 8 distinct'):
        optim.FusedAdamW(many)
    nine = [dict(params=[torch.nn.Parameter(torch.zeros(2))], lr=1e-3 * (i % 8 + 1)) for i in range(9)]
    assert len(optim.FusedAdamW(nine)._group_slots()[1]) == 8          # nine groups, eight sets
    e = torch.nn.Embedding(4, 2, sparse=True)
    e(torch.tensor([1])).sum().backward()
    with pytest.raises(RuntimeError, match='sparse gradients'):
        optim.FusedAdamW(e.parameters()).step()
    p.grad = torch.zeros(4)
    with pytest.raises(RuntimeError, match='no CPU path'):
        optim.FusedAdamW([p]).step()
    opt = optim.FusedAdamW([p])
    theirs = torch.optim.AdamW([p], amsgrad=True)
    with pytest.raises(ValueError, match='amsgrad'):
        opt.load_state_dict(theirs.state_dict())
    opt = optim.FusedAdamW([p])
    with pytest.raises(ValueError, match='norm_type'):
        optim.TrainingUpdate(opt, grad_clip=dict(max_norm=10, norm_type=1))
    with pytest.raises(ValueError, match='norm_type'):
        optim.TrainingUpdate(opt, grad_clip=dict(max_norm=10, norm_type=float('inf')))
    with pytest.raises(ValueError, match='loss_scale'):
        optim.TrainingUpdate(opt, loss_scale='static')
    with pytest.raises(ValueError, match='scale_window'):
        optim.TrainingUpdate(opt, loss_scale=dict(scale_window=100))
    with pytest.raises(TypeError, match='FusedAdamW'):
        optim.TrainingUpdate(torch.optim.AdamW([p]))
    model = _Block()
    with pytest.raises(ValueError, match="'SGD'"):
        optim.build_optimizer(model, dict(type='SGD', lr=0.1))
    with pytest.raises(ValueError, match='bias_lr_mult'):
        optim.build_optimizer(model, dict(type='AdamW', lr=0.1, paramwise_cfg=dict(bias_lr_mult=2.)))
    with pytest.raises(ValueError, match="'CosineAnnealing'"):
        optim.build_training_update(model, dict(optimizer=dict(type='AdamW'), lr_config=dict(policy='CosineAnnealing')), 10)
    with pytest.raises(ValueError, match='warmup'):
        optim.build_training_update(model, dict(optimizer=dict(type='AdamW'),
                                                lr_config=dict(policy='cyclic', warmup='linear')), 10)
