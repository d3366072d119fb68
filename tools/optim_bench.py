"""Times the training update (sst_amd.optim.TrainingUpdate: three launches of csrc/optim.hip) against the composition it
replaces - torch.amp.GradScaler + clip_grad_norm_(foreach=True) + torch.optim.AdamW (fused=True where this build accepts it,
else foreach) - on the parameters of shipped detectors after attach_heads(), in one process, the two paths alternating.

    python tools/optim_bench.py [--window 0.5] [--rounds 3] [--out profiles/optim/optim_bench.json]

Per detector (the headline config sst_waymoD5_1x_3class_8heads_v2 and fsd_waymoD1_1x) and path: milliseconds per update from
device events around a window of at least --window seconds of back-to-back updates (the median of --rounds windows), host
milliseconds per update (the time the same window takes to enqueue), kernel launches (torch.profiler, separate untimed call),
host synchronisations (tools/fg_sample_bench.count_syncs) and device allocations per update in steady state.  Both paths start
every update by restoring the same scaled gradients with one multi-tensor copy (GradScaler.unscale_ divides them in place); that
copy is timed alone as ``restore``.  Then the SST forward + backward + update step with each path on the 48 x 48 grid of
tests/test_gpu_sst_detector.py (two blocks: NOT the headline geometry), and the parity gaps of tests/test_gpu_optim.py's
one-step case."""
import argparse
import ast
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import _bench_common  # noqa: E402
from fg_sample_bench import count_syncs  # noqa: E402
import sst_amd  # noqa: E402
from sst_amd import optim  # noqa: E402

DEV = 'cuda:0'
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'configs')
OPT_CFG = dict(type='AdamW', lr=1e-5, betas=(0.9, 0.999), weight_decay=0.05, paramwise_cfg=dict(custom_keys={'norm': dict(decay_mult=0.)}))


def windows(fn, seconds, rounds):
    """-> (device ms per call, host ms per call): medians over ``rounds`` windows of at least ``seconds`` of back-to-back calls"""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    n = max(20, int(seconds / ((time.perf_counter() - t0) / 20)) + 1)
    dev, host = [], []
    for _ in range(rounds):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record()
        for _ in range(n):
            fn()
        stop.record()
        host.append((time.perf_counter() - t0) / n * 1e3)
        stop.synchronize()
        dev.append(start.elapsed_time(stop) / n)
    return sorted(dev)[len(dev) // 2], sorted(host)[len(host) // 2], n


def allocations(fn):
    fn()
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()['allocation.all.allocated']
    fn()
    return torch.cuda.memory_stats()['allocation.all.allocated'] - before


def torch_adamw(groups):
    try:
        return torch.optim.AdamW(groups, fused=True), 'fused'
    except (RuntimeError, ValueError, TypeError):
        return torch.optim.AdamW(groups, foreach=True), 'foreach'


def update_case(name, det, args):
    params = [p for p in det.parameters() if p.requires_grad]
    gen = torch.Generator(device=DEV).manual_seed(1)
    saved = [torch.randn(p.shape, device=DEV, generator=gen) * 0.5 for p in params]
    ours_opt = optim.build_optimizer(det, OPT_CFG)
    update = optim.TrainingUpdate(ours_opt, grad_clip=dict(max_norm=10, norm_type=2), loss_scale=32.0)
    theirs, kind = torch_adamw([dict(params=g['params'], lr=g['lr'], weight_decay=g['weight_decay']) for g in ours_opt.param_groups])
    scaler = torch.amp.GradScaler('cuda', init_scale=32.0)
    scaler.scale(torch.zeros(1, device=DEV))
    for p, g in zip(params, saved):
        p.grad = g.clone()
    grads = [p.grad for p in params]

    def restore():
        torch._foreach_copy_(grads, saved)

    def ours():
        restore()
        update.step()

    def composed():
        restore()
        scaler.unscale_(theirs)
        torch.nn.utils.clip_grad_norm_(params, 10.0, foreach=True)
        scaler.step(theirs)
        scaler.update(32.0)

    case = dict(detector=name, tensors=len(params), elements=int(sum(p.numel() for p in params)), torch_adamw=kind,
                stream_bytes_per_update=int(sum(p.numel() for p in params)) * 32)
    rounds = dict(ours=[], composed=[], restore=[])
    for _ in range(args.rounds):                    # alternate the paths: other work shares the machine
        for key, fn in (('ours', ours), ('composed', composed), ('restore', restore)):
            rounds[key].append(windows(fn, args.window, 1))
    for key, v in rounds.items():
        case[key + '_device_ms'] = round(sorted(x[0] for x in v)[len(v) // 2], 4)
        case[key + '_host_ms'] = round(sorted(x[1] for x in v)[len(v) // 2], 4)
        case[key + '_calls_per_window'] = v[0][2]
    case['ours_launches'] = _bench_common.count_launches(update.step, ours='optim_')
    counted = _bench_common.count_launches(lambda: (scaler.unscale_(theirs), torch.nn.utils.clip_grad_norm_(
        params, 10.0, foreach=True), scaler.step(theirs), scaler.update(32.0)), ours='optim_')
    case['composed_launches'] = counted      # 'ours': csrc/optim.hip's kernels (none on this path), 'torch': torch's
    case['ours_host_syncs'] = count_syncs(ours)
    case['composed_host_syncs'] = count_syncs(composed)
    case['ours_allocations'] = allocations(update.step)
    case['composed_allocations'] = allocations(lambda: (scaler.unscale_(theirs), torch.nn.utils.clip_grad_norm_(
        params, 10.0, foreach=True), scaler.step(theirs), scaler.update(32.0)))
    case['composed_over_ours_device'] = round((case['composed_device_ms'] - case['restore_device_ms'])
                                              / max(case['ours_device_ms'] - case['restore_device_ms'], 1e-6), 2)
    return case


def sst_step_case(args):
    """forward + backward + update of DynamicVoxelNet on the small grid of tests/test_gpu_sst_detector.py, each path"""
    import test_gpu_sst_detector as T
    import bench_workloads as BW
    clouds, centres = zip(*[BW.lidar_like_cloud(n, seed, DEV, half_extent=T.HALF - 0.3) for n, seed in ((3000, 3), (2600, 4))])
    boxes, labels = [], []
    for s, c in enumerate(centres):
        b = torch.zeros(4, 7)
        b[:, :2], b[:, 2] = c[:4, :2], -1.8
        b[:, 3:6] = torch.tensor([[2.0, 4.5, 1.7], [0.8, 0.9, 1.7], [0.8, 1.8, 1.7], [2.1, 4.8, 1.6]])
        boxes.append(b.to(DEV))
        labels.append(torch.tensor([0, 1, 2, 0], device=DEV))
    points = [c[:, :3].contiguous() for c in clouds]
    metas = [dict() for _ in points]
    out = dict(grid='48 x 48 windows grid of tests/test_gpu_sst_detector.py, 2 blocks, 2 frames')
    for path in ('ours', 'composed'):
        det = T._build('DynamicVoxelNet').train()
        params = [p for p in det.parameters() if p.requires_grad]
        opt = optim.build_optimizer(det, OPT_CFG)
        if path == 'ours':
            update = optim.TrainingUpdate(opt, grad_clip=dict(max_norm=10, norm_type=2), loss_scale=32.0)

            def step():
                opt.zero_grad(set_to_none=True)
                losses = T._flat(det.forward_train([p.clone() for p in points], metas, boxes, labels))
                update.scale(sum(v.sum() for v in losses.values())).backward()
                update.step()
        else:
            theirs, _ = torch_adamw([dict(params=g['params'], lr=g['lr'], weight_decay=g['weight_decay']) for g in opt.param_groups])
            scaler = torch.amp.GradScaler('cuda', init_scale=32.0)

            def step():
                theirs.zero_grad(set_to_none=True)
                losses = T._flat(det.forward_train([p.clone() for p in points], metas, boxes, labels))
                scaler.scale(sum(v.sum() for v in losses.values())).backward()
                scaler.unscale_(theirs)
                torch.nn.utils.clip_grad_norm_(params, 10.0, foreach=True)
                scaler.step(theirs)
                scaler.update(32.0)
        dev, host, n = windows(step, args.window, args.rounds)
        out[path + '_step_ms'], out[path + '_host_ms'], out[path + '_host_syncs'] = round(dev, 3), round(host, 3), count_syncs(step)
    return out


def parity_case():
    import optim_ref as R
    import test_gpu_optim as T
    out = {}
    for kind in ('mixed', 'tiny'):
        sizes = T._sizes(kind)
        max_norm = 10.0 if kind == 'mixed' else 5.0
        tensors = R.random_problem(5, sizes, T._groups_of(sizes), t=6, groups=T.GROUPS)
        want, norm, _ = R.update(tensors, T.GROUPS, max_norm=max_norm, scale=32.0)
        torchs, _ = R.torch_update(tensors, T.GROUPS, max_norm=max_norm, scale=32.0)
        run = T.Ours(tensors, T.GROUPS, grad_clip=dict(max_norm=max_norm, norm_type=2), loss_scale=32.0).step()
        worst_ours = worst_torch = 0.0
        for o, t, w in zip(run.result(), torchs, want):
            for go, gt, ww in zip(R.gaps(o, w[:3]), R.gaps(t, w[:3]), w[:3]):
                ulp = R.ulp32(abs(ww).max() if ww.size else 0.0)
                worst_ours, worst_torch = max(worst_ours, go / ulp), max(worst_torch, gt / ulp)
        out[kind] = dict(worst_gap_ulp_ours=round(worst_ours, 3), worst_gap_ulp_torch_cpu=round(worst_torch, 3),
                         total_norm_rel_gap=abs(float(run.update.grad_norm) - norm) / norm)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-step', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'optim_bench needs the GPU'
    count_syncs(lambda: None)      # the mode's own notice that it is a prototype appears once per process: not a step's
    res = dict(device=torch.cuda.get_device_name(0), window_s=args.window, rounds=args.rounds, updates=[])
    for name, rel in (('sst_waymoD5_1x_3class_8heads_v2', 'sst_refactor/sst_waymoD5_1x_3class_8heads_v2.model.py'),
                      ('fsd_waymoD1_1x', 'fsd/fsd_waymoD1_1x.model.py')):
        model = ast.literal_eval(open(os.path.join(GOLDEN, rel)).read())
        torch.manual_seed(0)
        det = sst_amd.build_detector(model).attach_heads().to(DEV)
        res['updates'].append(update_case(name, det, args))
        del det
    res['parity'] = parity_case()
    if not args.no_step:
        res['sst_step'] = sst_step_case(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
