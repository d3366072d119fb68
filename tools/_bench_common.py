"""What the head benchmarks (seg_loss_bench, center_head_bench, cluster_head_bench, roi_head_bench, anchor_head_bench) share:
the event-timed median and the profiler's launch counter."""
import torch


def median_ms(fn, iters, warmup=3):
    """-> (median, minimum) of ``iters`` event-timed calls in milliseconds, after ``warmup`` untimed ones"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    times.sort()
    return 0.5 * (times[(len(times) - 1) // 2] + times[len(times) // 2]), times[0]


def count_launches(fn, names_too=False, ours='', readback_names=None):
    """-> dict(ours, torch, memsets, copies) of one call (after one untimed call): device-side kernels whose name contains
    ``ours`` (the head's own), other kernels (torch's glue), memsets and copies; with ``readback_names`` (the names under which
    this profiler shows the copy of a host read) also device_to_host; with ``names_too`` the names; None without the profiler"""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]   # not the runtime calls on the host side
        if not names:
            return None
        kernels = [n for n in names if 'memcpy' not in n.lower() and 'memset' not in n.lower()]
        own = [n for n in kernels if ours in n]
        out = dict(ours=len(own), torch=len(kernels) - len(own), memsets=len([n for n in names if 'memset' in n.lower()]),
                   copies=len([n for n in names if 'memcpy' in n.lower()]))
        if readback_names is not None:
            out['device_to_host'] = len([n for n in names if n in readback_names or 'dtoh' in n.lower()])
        if names_too:
            out['names'] = [n.replace('(anonymous namespace)::', '')[:64] for n in names]
        return out
    except Exception:
        return None
