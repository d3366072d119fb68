"""The training update behind the loss: unscale, gradient norm, clip, AdamW and the loss-scale bookkeeping in three launches
(csrc/optim.hip), with the schedules and the config reading that go with it.

The reference's runner does this through mmcv's hooks: ``OptimizerHook`` / ``Fp16OptimizerHook`` (mmcv/runner/hooks/optimizer.py)
call ``clip_grad_norm_`` and ``optimizer.step()``, ``DefaultOptimizerConstructor`` (mmcv/runner/optimizer/default_constructor.py)
builds the parameter groups, ``CyclicLrUpdaterHook`` / ``CyclicMomentumUpdaterHook`` write the learning rate and the momentum
before every iteration.  Every config of configs/{sst,sst_refactor,fsd,fsdv2} asks for AdamW, an L2 gradient clip and the cyclic
policy; the SST configs add ``fp16 = dict(loss_scale=32.0)``.

    optimizer = build_optimizer(model, cfg['optimizer'])                 # FusedAdamW, groups as mmcv builds them
    update = TrainingUpdate(optimizer, grad_clip=dict(max_norm=10, norm_type=2), loss_scale=32.0, reducer=reducer)
    lr = CyclicLr(optimizer, max_iters, target_ratio=(100, 1e-3), step_ratio_up=0.1)
    for it in range(max_iters):
        lr.step(it)
        optimizer.zero_grad()
        update.scale(loss_fn()).backward()
        update.step()                                                    # no host read; update.grad_norm is a device tensor

There is no CPU path: ``step()`` on CPU parameters raises.  Construction, the groups, ``state_dict()`` and the schedules are host
work and run anywhere.
"""
import copy
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib

MAX_GROUPS = 8
_TENSOR_DTYPE = np.dtype([('p', '<u8'), ('g', '<u8'), ('m', '<u8'), ('v', '<u8'), ('numel', '<i8'), ('group', '<i4'),
                          ('slot', '<i4')])
_CHUNK_DTYPE = np.dtype([('start', '<i8'), ('tensor', '<i4'), ('count', '<i4')])
SCALE_NONE, SCALE_FIXED, SCALE_DYNAMIC = 0, 1, 2


def _align(n, a):
    return (n + a - 1) // a * a


def chunk_table(numels, chunk):
    """the chunk entries (start, tensor, count) of tensors with these element counts: every tensor cut into slices of at most
    ``chunk`` elements, tensor by tensor; a tensor of numel 0 has none"""
    numels = np.asarray(numels, dtype=np.int64)
    per = (numels + chunk - 1) // chunk
    out = np.zeros(int(per.sum()), dtype=_CHUNK_DTYPE)
    if len(out):
        tensor = np.repeat(np.arange(len(numels), dtype=np.int64), per)
        first = np.cumsum(per) - per
        k = np.arange(len(out), dtype=np.int64) - first[tensor]
        out['tensor'] = tensor
        out['start'] = k * chunk
        out['count'] = np.minimum(numels[tensor] - k * chunk, chunk)
    return out


class DeviceRecord(object):
    """the small device record of an update (include/sst_amd.h: sst_optim_step_f32): norm, coefficient, found_inf, scale, tracker
    and the count of skipped steps, each a view that is read only when the caller asks"""

    def __init__(self, device, init_scale=1.0):
        nbytes = _lib.load().sst_optim_record_bytes()
        self.buffer = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        f32, i32 = self.buffer.view(torch.float32), self.buffer.view(torch.int32)
        self.total_norm = self.buffer.view(torch.float64)[0]
        self.clip_coef, self.inv_scale, self.scale = f32[2], f32[3], f32[4]
        self.found_inf, self.growth_tracker, self.skipped_steps = i32[5], i32[6], i32[7]
        self.clip_coef64 = self.buffer.view(torch.float64)[4]       # the coefficient before its rounding to fp32
        self.scale.fill_(float(init_scale))


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (decoupled weight decay) whose step is the three launches of csrc/optim.hip for all parameters.

    ``param_groups``, ``state_dict()`` / ``load_state_dict()`` (``step``, ``exp_avg``, ``exp_avg_sq`` per parameter index) and
    ``zero_grad()`` are torch's.  A parameter whose ``grad`` is None is left out of the step and its counter does not move.  The
    moments of all parameters live in one allocation at 16-byte aligned offsets, the step counters in one fp32 device array
    (torch's own type for ``step``); the work table in device memory is rebuilt only when a ``data_ptr`` changed.

    Refused by name: amsgrad, maximize, parameters that are not float32 or not contiguous, sparse gradients, parameters on several
    devices, more than 8 distinct hyper-parameter sets."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False):
        if amsgrad:
            raise ValueError('FusedAdamW: amsgrad is not supported')
        if maximize:
            raise ValueError('FusedAdamW: maximize is not supported')
        if not 0.0 <= lr:
            raise ValueError(f'FusedAdamW: invalid lr {lr}')
        if not 0.0 <= eps:
            raise ValueError(f'FusedAdamW: invalid eps {eps}')
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f'FusedAdamW: invalid betas {betas}')
        if not 0.0 <= weight_decay:
            raise ValueError(f'FusedAdamW: invalid weight_decay {weight_decay}')
        # the keys of torch.optim.AdamW's groups, so that a state_dict() of either loads into the other
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        self._plist = None          # parameters in state_dict index order
        self._moments = None
        self._steps = None
        self._adopt = True          # state entries that are not views of the flat buffers wait to be copied in
        self._table_key = None
        self._pins = []
        self._record = None
        super().__init__(params, defaults)
        self._group_slots()

    # ------------------------------------------------------------------------------------------------------------------
    # host bookkeeping
    # ------------------------------------------------------------------------------------------------------------------
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        if group.get('amsgrad', False):
            raise ValueError('FusedAdamW: amsgrad is not supported')
        if group.get('maximize', False):
            raise ValueError('FusedAdamW: maximize is not supported')
        for p in group['params']:
            if p.dtype != torch.float32:
                raise TypeError(f'FusedAdamW: non-fp32 parameter ({p.dtype}); the update is fp32 only')
            if not p.is_contiguous():
                raise ValueError('FusedAdamW: non-contiguous parameter')
        devices = {p.device for g in self.param_groups for p in g['params']}
        if len(devices) > 1:
            raise ValueError(f'FusedAdamW: parameters on several devices ({sorted(str(d) for d in devices)})')
        self._plist = None
        self._table_key = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            if group.get('amsgrad', False):
                raise ValueError('FusedAdamW: amsgrad is not supported')
            if group.get('maximize', False):
                raise ValueError('FusedAdamW: maximize is not supported')
        self._adopt = True
        self._table_key = None

    def state_dict(self):
        """torch's layout, as a snapshot: ``step``, ``exp_avg`` and ``exp_avg_sq`` are copies (one clone of the counters, one of
        the moment buffer).  The live entries are views of the optimizer's flat buffers, and torch's load_state_dict hands a
        tensor of the right dtype and device on without copying it: an optimizer that loaded the live views would update
        this one's moments and advance its counters."""
        sd = super().state_dict()
        if self._steps is not None:
            steps, moments = self._steps.clone(), self._moments.clone()
            m_off = {id(v): v.storage_offset() for v in self._m}
            v_off = {id(v): v.storage_offset() for v in self._v}
            live = {id(v): i for i, v in enumerate(self._step_views)}

            def snapshot(st):
                if id(st.get('step')) not in live or id(st.get('exp_avg')) not in m_off:
                    return st                     # loaded and not stepped yet: not views of the flat buffers
                m, v = st['exp_avg'], st['exp_avg_sq']
                mo, vo = m_off[id(m)], v_off[id(v)]
                return {**st, 'step': steps[live[id(st['step'])]], 'exp_avg': moments[mo:mo + m.numel()].view_as(m),
                        'exp_avg_sq': moments[vo:vo + v.numel()].view_as(v)}
            sd['state'] = {k: snapshot(st) for k, st in sd['state'].items()}
        return sd

    def _group_slots(self):
        """hyper-parameter slot of every param_group and the slots' (lr, wd, b1, b2, eps): the group index while there are at
        most 8 groups, the distinct sets in order of appearance otherwise"""
        sets = [(float(g['lr']), float(g['weight_decay']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']))
                for g in self.param_groups]
        if len(sets) <= MAX_GROUPS:
            return list(range(len(sets))), sets
        distinct = {}
        slots = [distinct.setdefault(s, len(distinct)) for s in sets]
        if len(distinct) > MAX_GROUPS:
            raise ValueError(f'FusedAdamW: more than {MAX_GROUPS} distinct hyper-parameter sets ({len(distinct)})')
        return slots, list(distinct)

    def _params(self):
        if self._plist is None:
            self._plist = [p for g in self.param_groups for p in g['params']]
            self._pgroup = [gi for gi, g in enumerate(self.param_groups) for _ in g['params']]
        return self._plist

    def _ensure_state(self):
        params = self._params()
        if not params[0].is_cuda:
            self._refuse_sparse()
            raise RuntimeError('FusedAdamW: parameters must be CUDA/HIP tensors (no CPU path in this library)')
        dev = params[0].device
        if self._steps is None or self._steps.numel() != len(params):
            lib = _lib.load()
            offs, total = [], 0
            for p in params:
                offs.append(total)
                total += _align(p.numel(), 4)          # 16-byte aligned offsets
            moments = torch.zeros(2 * max(total, 4), dtype=torch.float32, device=dev)
            steps = torch.zeros(len(params), dtype=torch.float32, device=dev)
            half = max(total, 4)
            self._m = [moments[o:o + p.numel()].view_as(p) for o, p in zip(offs, params)]
            self._v = [moments[half + o:half + o + p.numel()].view_as(p) for o, p in zip(offs, params)]
            self._step_views = [steps[i] for i in range(len(params))]
            self._moments, self._steps, self._adopt = moments, steps, True
            self._chunk = lib.sst_optim_chunk_elems()
            # capacities for every parameter having a gradient: nothing is allocated on a later step
            n_chunks = int(sum(-(-p.numel() // self._chunk) for p in params))
            self._chunk_off = _align(len(params) * _TENSOR_DTYPE.itemsize, 256)
            self._table_bytes = self._chunk_off + max(n_chunks, 1) * _CHUNK_DTYPE.itemsize
            self._table = torch.zeros(self._table_bytes, dtype=torch.uint8, device=dev)
            self._workspace = _lib.workspace(lib.sst_optim_workspace_bytes(len(params)), dev)
            self._table_key = None
            self._pins = []
        if self._adopt:
            # state from before the buffers existed, or loaded: move it into the flat buffers and point the entries at them
            for i, p in enumerate(params):
                st = self.state.get(p)
                if not st:
                    continue
                if st['exp_avg'] is not self._m[i]:
                    self._m[i].copy_(st['exp_avg'])
                    self._v[i].copy_(st['exp_avg_sq'])
                    self._step_views[i].copy_(torch.as_tensor(st['step'], dtype=torch.float32))
                st['exp_avg'], st['exp_avg_sq'], st['step'] = self._m[i], self._v[i], self._step_views[i]
            self._adopt = False
        return dev

    def _refuse_sparse(self):
        if any(p.grad is not None and p.grad.is_sparse for p in self._params()):
            raise RuntimeError('FusedAdamW: sparse gradients are not supported')

    def _pinned(self):
        """a pinned staging buffer whose last upload has completed (or a new one: the wait is never taken)"""
        for pin, event in self._pins:
            if event.query():
                return pin, event
        pin = torch.empty(self._table_bytes, dtype=torch.uint8, pin_memory=True)
        event = torch.cuda.Event()
        self._pins.append((pin, event))
        return pin, event

    def _sync_table(self, slots):
        params = self._params()
        pptr = [p.data_ptr() for p in params]
        try:
            gptr = [None if p.grad is None else p.grad.data_ptr() for p in params]   # an empty tensor's is 0
        except RuntimeError:
            self._refuse_sparse()
            raise
        key = (pptr, gptr, slots)
        if key == self._table_key:
            return
        have = [i for i, g in enumerate(gptr) if g is not None]
        for i in have:
            g, p = params[i].grad, params[i]
            if g.is_sparse:
                raise RuntimeError('FusedAdamW: sparse gradients are not supported')
            if g.dtype != torch.float32 or g.device != p.device or not g.is_contiguous() or g.numel() != p.numel():
                raise RuntimeError('FusedAdamW: a gradient must be a contiguous float32 tensor of its parameter\'s size and device')
            if p not in self.state or not self.state[p]:
                self.state[p] = {'step': self._step_views[i], 'exp_avg': self._m[i], 'exp_avg_sq': self._v[i]}
        tensors = np.zeros(len(have), dtype=_TENSOR_DTYPE)
        tensors['p'] = [pptr[i] for i in have]
        tensors['g'] = [gptr[i] for i in have]
        tensors['m'] = [self._m[i].data_ptr() for i in have]
        tensors['v'] = [self._v[i].data_ptr() for i in have]
        tensors['numel'] = [params[i].numel() for i in have]
        tensors['group'] = [slots[self._pgroup[i]] for i in have]
        tensors['slot'] = have
        chunks = chunk_table(tensors['numel'], self._chunk)
        pin, event = self._pinned()
        host = pin.numpy()
        host[:tensors.nbytes] = tensors.view(np.uint8)
        host[self._chunk_off:self._chunk_off + chunks.nbytes] = chunks.view(np.uint8)
        used = self._chunk_off + chunks.nbytes
        self._table[:used].copy_(pin[:used], non_blocking=True)
        event.record()
        self._n_tensors, self._n_chunks = len(tensors), len(chunks)
        self._table_key = key

    # ------------------------------------------------------------------------------------------------------------------
    # the step
    # ------------------------------------------------------------------------------------------------------------------
    def _launch(self, record, max_norm=-1.0, scale_mode=SCALE_NONE, skip_nonfinite=False, growth_factor=2.0, backoff_factor=0.5,
                growth_interval=2000):
        dev = self._ensure_state()
        slots, sets = self._group_slots()
        with torch.cuda.device(dev):
            self._sync_table(slots)
            h = _lib.OptimHyper()
            for s, (lr, wd, b1, b2, eps) in enumerate(sets):
                h.lr[s], h.wd[s], h.b1[s], h.b2[s], h.eps[s] = lr, wd, b1, b2, eps
            h.max_norm, h.growth_factor, h.backoff_factor = float(max_norm), float(growth_factor), float(backoff_factor)
            h.growth_interval, h.scale_mode, h.skip_nonfinite, h.n_groups = int(growth_interval), int(scale_mode), \
                int(bool(skip_nonfinite)), len(sets)
            base = self._table.data_ptr()
            rc = _lib.load().sst_optim_step_f32(ctypes.c_void_p(base), self._n_tensors, ctypes.c_void_p(base + self._chunk_off),
                                                self._n_chunks, ctypes.byref(h), _lib.ptr(self._steps), _lib.ptr(record.buffer),
                                                _lib.ptr(self._workspace), _lib.stream_ptr())
        _lib.check(rc, 'sst_optim_step_f32')

    @torch.no_grad()
    def step(self, closure=None):
        """one AdamW step of every parameter that has a gradient: no clipping, no loss scale, a NaN goes through as in torch"""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        dev = self._ensure_state()
        if self._record is None:
            self._record = DeviceRecord(dev)
        self._launch(self._record)
        return loss


def build_optimizer(model, cfg):
    """the configs' ``optimizer`` dictionary -> FusedAdamW with the parameter groups of mmcv's DefaultOptimizerConstructor
    (mmcv/runner/optimizer/default_constructor.py, 1.3.9): the keys of ``paramwise_cfg.custom_keys`` sorted alphabetically, then
    by length with the longest first; the first key that is a substring of a parameter's full name gives its ``lr_mult`` /
    ``decay_mult``.  Parameters with equal settings share a group (mmcv makes one group per parameter: the same update)."""
    cfg = copy.deepcopy(dict(cfg))
    kind = cfg.pop('type', 'AdamW')
    if kind != 'AdamW':
        raise ValueError(f'build_optimizer: optimizer type {kind!r} is not supported (AdamW only)')
    paramwise = cfg.pop('paramwise_cfg', None) or {}
    other = sorted(set(paramwise) - {'custom_keys'})
    if other:
        raise ValueError(f'build_optimizer: paramwise_cfg key {other[0]!r} is not supported (custom_keys only)')
    custom = paramwise.get('custom_keys', {}) or {}
    for key, val in custom.items():
        extra = sorted(set(val) - {'lr_mult', 'decay_mult'})
        if extra:
            raise ValueError(f'build_optimizer: custom_keys[{key!r}] entry {extra[0]!r} is not supported (lr_mult, decay_mult)')
    base_lr, base_wd = cfg.get('lr', 1e-3), cfg.get('weight_decay', 1e-2)
    keys = sorted(sorted(custom), key=len, reverse=True)
    groups = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        lr, wd = base_lr, base_wd
        for key in keys:
            if key in name:
                lr = base_lr * custom[key].get('lr_mult', 1.)
                wd = base_wd * custom[key].get('decay_mult', 1.)
                break
        groups.setdefault((lr, wd), []).append(p)
    if not groups:
        raise ValueError('build_optimizer: the model has no parameter that requires a gradient')
    return FusedAdamW([dict(params=ps, lr=lr, weight_decay=wd) for (lr, wd), ps in groups.items()], **cfg)


class TrainingUpdate(object):
    """What mmcv's OptimizerHook / Fp16OptimizerHook do after the loss: ``scale(loss).backward()`` then ``step()``.

    grad_clip: ``dict(max_norm=..., norm_type=2)`` or None.  loss_scale: a float (held fixed, as Fp16OptimizerHook holds it),
    ``'dynamic'`` or a dict of torch.amp.GradScaler's arguments (init_scale, growth_factor, backoff_factor, growth_interval), or
    None.  With a loss scale a step whose gradients are not finite is skipped; without one only if ``skip_nonfinite`` (the
    reference's plain hook lets a NaN through).  ``grad_norm``, ``clip_coef``, ``found_inf``, ``scale``, ``growth_tracker`` and
    ``skipped_steps`` are device tensors of the last step, read only when the caller reads them."""

    def __init__(self, optimizer, grad_clip=None, loss_scale=None, reducer=None, skip_nonfinite=False):
        if not isinstance(optimizer, FusedAdamW):
            raise TypeError('TrainingUpdate: the optimizer must be a FusedAdamW')
        self.optimizer, self.reducer = optimizer, reducer
        self.max_norm = -1.0
        if grad_clip is not None:
            clip = dict(grad_clip)
            norm_type = clip.pop('norm_type', 2)
            if float(norm_type) != 2.0:
                raise ValueError(f'TrainingUpdate: grad_clip norm_type={norm_type!r} is not supported (2 only)')
            max_norm = clip.pop('max_norm')
            if clip:
                raise ValueError(f'TrainingUpdate: grad_clip key {sorted(clip)[0]!r} is not supported')
            if not max_norm >= 0:
                raise ValueError(f'TrainingUpdate: invalid max_norm {max_norm}')
            self.max_norm = float(max_norm)
        self.growth_factor, self.backoff_factor, self.growth_interval = 2.0, 0.5, 2000
        if loss_scale is None:
            self.scale_mode, self.init_scale = SCALE_NONE, 1.0
        elif isinstance(loss_scale, (int, float)) and not isinstance(loss_scale, bool):
            self.scale_mode, self.init_scale = SCALE_FIXED, float(loss_scale)
        elif loss_scale == 'dynamic' or isinstance(loss_scale, dict):
            args = {} if loss_scale == 'dynamic' else dict(loss_scale)
            self.scale_mode = SCALE_DYNAMIC
            self.init_scale = float(args.pop('init_scale', 2.0 ** 16))
            self.growth_factor = float(args.pop('growth_factor', 2.0))
            self.backoff_factor = float(args.pop('backoff_factor', 0.5))
            self.growth_interval = int(args.pop('growth_interval', 2000))
            if args:
                raise ValueError(f'TrainingUpdate: loss_scale key {sorted(args)[0]!r} is not supported')
        else:
            raise ValueError(f'TrainingUpdate: loss_scale {loss_scale!r} is not a number, \'dynamic\', a dict or None')
        if not self.init_scale > 0:
            raise ValueError(f'TrainingUpdate: invalid loss scale {self.init_scale}')
        self.skip_nonfinite = self.scale_mode != SCALE_NONE or bool(skip_nonfinite)
        self._record = None

    @property
    def record(self):
        if self._record is None:
            params = self.optimizer._params()
            if not params[0].is_cuda:
                raise RuntimeError('TrainingUpdate: parameters must be CUDA/HIP tensors (no CPU path in this library)')
            self._record = DeviceRecord(params[0].device, self.init_scale)
        return self._record

    grad_norm = property(lambda self: self.record.total_norm)
    clip_coef = property(lambda self: self.record.clip_coef)
    found_inf = property(lambda self: self.record.found_inf)
    scale_tensor = property(lambda self: self.record.scale)
    growth_tracker = property(lambda self: self.record.growth_tracker)
    skipped_steps = property(lambda self: self.record.skipped_steps)

    def scale(self, loss):
        """the loss times the device-resident scale (the loss itself without a loss scale)"""
        if self.scale_mode == SCALE_NONE:
            return loss
        return loss * self.record.scale

    def get_scale(self):
        """the scale as a device tensor"""
        return self.record.scale

    @torch.no_grad()
    def step(self):
        if self.reducer is not None:
            self.reducer.finish()
        self.optimizer._launch(self.record, self.max_norm, self.scale_mode, self.skip_nonfinite, self.growth_factor,
                               self.backoff_factor, self.growth_interval)


def annealing_cos(start, end, factor):
    """mmcv's annealing_cos: from ``start`` (factor 0) to ``end`` (factor 1) along half a cosine"""
    return end + 0.5 * (start - end) * (math.cos(math.pi * factor) + 1)


def cyclic_value(base, it, max_iters, target_ratio, cyclic_times=1, step_ratio_up=0.4):
    """the value of mmcv's cyclic policy at iteration ``it``"""
    per = max_iters // cyclic_times
    up = int(step_ratio_up * per)
    it = it % per
    r0, r1 = target_ratio
    if it < up:
        return annealing_cos(base, base * r0, it / up)
    return annealing_cos(base * r0, base * r1, (it - up) / (per - up))


class _Cyclic(object):
    def __init__(self, optimizer, max_iters, target_ratio, cyclic_times=1, step_ratio_up=0.4):
        if isinstance(target_ratio, (int, float)):
            target_ratio = (target_ratio, target_ratio / 1e5)
        if len(target_ratio) != 2:
            raise ValueError('cyclic schedule: target_ratio is a pair (peak ratio, final ratio)')
        if not 0 <= step_ratio_up < 1.0:
            raise ValueError('cyclic schedule: step_ratio_up must be in [0, 1)')
        if max_iters // cyclic_times < 1:
            raise ValueError('cyclic schedule: max_iters // cyclic_times must be at least 1')
        self.optimizer, self.max_iters, self.target_ratio = optimizer, int(max_iters), tuple(target_ratio)
        self.cyclic_times, self.step_ratio_up = int(cyclic_times), float(step_ratio_up)
        self.base = [self._read(g) for g in optimizer.param_groups]

    def values(self, it):
        return [cyclic_value(b, it, self.max_iters, self.target_ratio, self.cyclic_times, self.step_ratio_up) for b in self.base]

    def step(self, it):
        """write iteration ``it``'s value into every group (call before the iteration's update)"""
        for group, value in zip(self.optimizer.param_groups, self.values(it)):
            self._write(group, value)


class CyclicLr(_Cyclic):
    """mmcv's CyclicLrUpdaterHook (mmcv/runner/hooks/lr_updater.py, 1.3.9) per iteration: ``per = max_iters // cyclic_times``,
    ``up = int(step_ratio_up * per)``, ``it %= per``; below ``up`` the rate anneals from ``base`` to ``base * target_ratio[0]`` with
    progress ``it / up``, from there to ``base * target_ratio[1]`` with progress ``(it - up) / (per - up)``;
    ``anneal(a, b, f) = b + 0.5 (a - b) (cos(pi f) + 1)``.  ``base`` is each group's ``lr`` at construction."""

    @staticmethod
    def _read(group):
        return float(group['lr'])

    @staticmethod
    def _write(group, value):
        group['lr'] = value


class CyclicMomentum(_Cyclic):
    """mmcv's CyclicMomentumUpdaterHook (mmcv/runner/hooks/momentum_updater.py, 1.3.9): the schedule of CyclicLr applied to
    ``betas[0]``, whose value at construction is the base."""

    @staticmethod
    def _read(group):
        return float(group['betas'][0])

    @staticmethod
    def _write(group, value):
        group['betas'] = (value, group['betas'][1])


def _merge(base, new):
    """mmcv.Config's merge: dictionaries merge recursively, ``_delete_=True`` replaces"""
    out = copy.deepcopy(base)
    for k, v in new.items():
        if isinstance(v, dict) and isinstance(out.get(k), dict) and not v.get('_delete_', False):
            out[k] = _merge(out[k], v)
        else:
            out[k] = copy.deepcopy({kk: vv for kk, vv in v.items() if kk != '_delete_'} if isinstance(v, dict) else v)
    return out


def resolve_config(text, base_dir=None, name='<config>'):
    """a config's text as mmcv.Config.fromfile reads it: run the text, resolve its ``_base_`` files (paths relative to
    ``base_dir``) first"""
    ns = {}
    exec(compile(text, name, 'exec'), ns)
    cfg = {k: v for k, v in ns.items() if not k.startswith('__') and not callable(v) and not isinstance(v, type(os))}
    bases = cfg.pop('_base_', [])
    merged = {}
    for b in ([bases] if isinstance(bases, str) else bases):
        if base_dir is None:
            raise ValueError('resolve_config: the text names _base_ files; pass base_dir (the directory of the config)')
        path = os.path.normpath(os.path.join(base_dir, b))
        with open(path) as f:
            merged = _merge(merged, resolve_config(f.read(), os.path.dirname(path), path))
    return _merge(merged, cfg)


def _schedule(kind, cls, cfg, optimizer, max_iters):
    if cfg is None:
        return None
    cfg = dict(cfg)
    policy = cfg.pop('policy', None)
    if policy != 'cyclic':
        raise ValueError(f'build_training_update: {kind} policy {policy!r} is not supported (cyclic only)')
    if cfg.pop('by_epoch', False):
        raise ValueError(f'build_training_update: {kind} by_epoch=True is not supported')
    if cfg.pop('warmup', None) is not None:
        raise ValueError(f'build_training_update: {kind} warmup is not supported')
    args = {k: cfg.pop(k) for k in ('target_ratio', 'cyclic_times', 'step_ratio_up') if k in cfg}
    if cfg:
        raise ValueError(f'build_training_update: {kind} key {sorted(cfg)[0]!r} is not supported')
    return cls(optimizer, max_iters, **args)


def build_training_update(model, cfg, max_iters, reducer=None, base_dir=None):
    """``optimizer``, ``optimizer_config``, ``lr_config``, ``momentum_config`` and ``fp16`` of a shipped config -> (TrainingUpdate,
    [schedules]).  ``cfg``: the resolved dictionary, or the config's text (its ``_base_`` files are read from ``base_dir``).  Call
    ``schedule.step(it)`` for every schedule before iteration ``it``."""
    if isinstance(cfg, str):
        cfg = resolve_config(cfg, base_dir)
    if 'optimizer' not in cfg:
        raise ValueError('build_training_update: the config has no optimizer')
    optimizer = build_optimizer(model, cfg['optimizer'])
    ocfg = dict(cfg.get('optimizer_config') or {})
    grad_clip = ocfg.pop('grad_clip', None)
    if ocfg:
        raise ValueError(f'build_training_update: optimizer_config key {sorted(ocfg)[0]!r} is not supported')
    fp16 = cfg.get('fp16')
    loss_scale = None
    if fp16 is not None:
        fp16 = dict(fp16)
        loss_scale = fp16.pop('loss_scale', 512.)       # Fp16OptimizerHook's default
        if fp16:
            raise ValueError(f'build_training_update: fp16 key {sorted(fp16)[0]!r} is not supported')
    update = TrainingUpdate(optimizer, grad_clip=grad_clip, loss_scale=loss_scale, reducer=reducer)
    schedules = [s for s in (_schedule('lr_config', CyclicLr, cfg.get('lr_config'), optimizer, max_iters),
                             _schedule('momentum_config', CyclicMomentum, cfg.get('momentum_config'), optimizer, max_iters))
                 if s is not None]
    return update, schedules
