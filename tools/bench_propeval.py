#!/usr/bin/env python3
"""Time the two streaming kernels of the JHMDB / VIP evaluation path (csrc/propeval.hip) at their full sizes and print
their share of the HBM streaming roof:

* vfs_heatmap_topk at the JHMDB size: 40 frames x 15 key points x 240 x 320 fp32 maps, topk 5 (bytes = 4*N*H*W)
* vfs_label_counts at a VIP-like size: 8 frames of 720 x 1280, 20 classes, 5 % ignored (bytes = 2*n)

What is timed: device events around back-to-back launches issued from Python through ctypes, after warm-up, over enough
repetitions to fill a few hundred milliseconds, divided by the launch count = TIME PER LAUNCH.  Issuing a launch from
Python costs some 20 us of host time, so for a kernel shorter than that the figure is the submission rate, an upper bound
on the kernel's time.  The kernel's own time comes from a profiler run of this script:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o propeval -- python tools/bench_propeval.py --no-numpy
and `--kernel-stats DIR/.../propeval_kernel_stats.csv` on a later (unprofiled) run merges its averages into the report.
The inputs rotate over several copies (more than the 256 MB last-level cache holds) so that a repetition reads HBM, not
the cache its predecessor filled.  As context only: the numpy time of the reference's expressions (np.argsort over every map;
three np.histogram calls per frame) on this host.

Usage: python tools/bench_propeval.py [--out profiles/propeval_bench.json] [--no-numpy] [--kernel-stats FILE.csv]"""
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit('/tools/', 1)[0])
from vfs_amd._lib import get_lib  # noqa: E402

HBM_ACHIEVABLE_TBS = 6.29       # float4 copy on the MI355X (8.0 TB/s on the data sheet)
TARGET_MS = 300.0


def _time(fns, target_ms=TARGET_MS):
    """fns: the same launch on rotating inputs -> ms per launch"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for fn in fns:
        fn()
    e1.record()
    torch.cuda.synchronize()
    rounds = max(1, int(target_ms / max(e0.elapsed_time(e1), 1e-3)))
    e0.record()
    for _ in range(rounds):
        for fn in fns:
            fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (rounds * len(fns)), rounds * len(fns)


KERNEL_STATS = {}      # --kernel-stats: {kernel function name prefix: (calls, average ns)} of a rocprofv3 run of this script


def _load_kernel_stats(path):
    import csv
    with open(path) as f:
        for row in csv.DictReader(f):
            KERNEL_STATS[row['Name'].replace('void ', '')] = (int(row['Calls']), float(row['AverageNs']))


def _report(name, function, ms, launches, nbytes, extra):
    tbs = nbytes / (ms * 1e-3) / 1e12
    res = dict(kernel=name, time_per_launch_ms=round(ms, 5), launches_timed=launches, algorithmic_bytes=nbytes,
               bytes_over_time_per_launch_TBs=round(tbs, 3), share_of_streaming_roof_per_launch=round(tbs / HBM_ACHIEVABLE_TBS, 3),
               **extra)
    hit = [v for k, v in KERNEL_STATS.items() if k.startswith(function)]
    if hit:
        calls, ns = hit[0]
        ktbs = nbytes / (ns * 1e-9) / 1e12
        res.update(kernel_time_ms_rocprofv3=round(ns * 1e-6, 5), rocprofv3_calls=calls, bytes_over_kernel_time_TBs=round(ktbs, 3),
                   share_of_streaming_roof_kernel=round(ktbs / HBM_ACHIEVABLE_TBS, 3))
    else:
        res['kernel_time_ms_rocprofv3'] = 'not measured'
    return res


def bench_topk(lib, dev, with_numpy):
    T, K, H, W, topk, copies = 40, 15, 240, 320, 5, 3
    N = T * K
    g = torch.Generator(device=dev).manual_seed(0)
    maps = [torch.rand(N, H * W, generator=g, device=dev) for _ in range(copies)]
    vals = torch.empty(N, topk, device=dev)
    idx = torch.empty(N, topk, dtype=torch.int32, device=dev)
    minv = torch.empty(N, device=dev)
    flags = torch.empty(N, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    ms, n = _time([lambda m=m: lib.heatmap_topk(m, vals, idx, minv, flags, N, H, W, topk, s) for m in maps])
    extra = dict(shape=[T, K, H, W], topk=topk, workgroups=N, input_copies_rotated=copies)
    if with_numpy:
        host = maps[0].cpu().numpy().reshape(T, K, -1)
        t0 = time.perf_counter()
        ind = np.argsort(host, axis=-1)[..., -topk:]
        np.take_along_axis(host, ind, axis=-1)
        extra['numpy_argsort_ms_context_only'] = round((time.perf_counter() - t0) * 1e3, 1)
    else:
        extra['numpy_argsort_ms_context_only'] = 'not measured'
    return _report('vfs_heatmap_topk', 'heatmap_topk_kernel<5>', ms, n, 4 * N * H * W, extra)


def bench_counts(lib, dev, with_numpy):
    T, H, W, nc, copies = 8, 720, 1280, 20, 20
    n = T * H * W
    g = torch.Generator(device=dev).manual_seed(1)
    pairs = []
    for _ in range(copies):
        coarse = torch.randint(0, nc, (T, H // 8, W // 8), generator=g, device=dev, dtype=torch.uint8)
        gt = coarse.repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()
        pred = torch.where(torch.rand(T, H, W, generator=g, device=dev) < 0.2, torch.roll(gt, 3, 2), gt).contiguous()
        gt[torch.rand(T, H, W, generator=g, device=dev) < 0.05] = 255
        pairs.append((pred, gt))
    counts = torch.zeros(nc, 3, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    ms, launches = _time([lambda p=p, q=q: lib.label_counts(p, q, counts, n, nc, 255, s) for p, q in pairs])
    extra = dict(shape=[T, H, W], num_classes=nc, ignored_fraction=0.05, input_copies_rotated=copies)
    if with_numpy:
        p, q = pairs[0][0].cpu().numpy(), pairs[0][1].cpu().numpy()
        bins = np.arange(nc + 1)
        t0 = time.perf_counter()
        for f in range(T):
            mask = q[f] != 255
            pl, ll = p[f][mask], q[f][mask]
            np.histogram(pl[pl == ll], bins=bins), np.histogram(pl, bins=bins), np.histogram(ll, bins=bins)
        extra['numpy_histogram_ms_context_only'] = round((time.perf_counter() - t0) * 1e3, 1)
    else:
        extra['numpy_histogram_ms_context_only'] = 'not measured'
    return _report('vfs_label_counts', 'label_counts_kernel', ms, launches, 2 * n, extra)


def main():
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    with_numpy = '--no-numpy' not in sys.argv
    if '--kernel-stats' in sys.argv:
        _load_kernel_stats(sys.argv[sys.argv.index('--kernel-stats') + 1])
    dev = torch.device('cuda:0')
    lib = get_lib()
    res = dict(device=torch.cuda.get_device_name(0), streaming_roof_TBs=HBM_ACHIEVABLE_TBS,
               roof_source='float4 copy, MI355X micro-architecture notes',
               timing='time_per_launch: device events around back-to-back launches from Python / launch count (an upper bound on '
                      'the kernel time); kernel_time: rocprofv3 --kernel-trace --stats average of a profiled run of this script',
               kernels=[bench_topk(lib, dev, with_numpy), bench_counts(lib, dev, with_numpy)])
    print(json.dumps(res))
    if out:
        with open(out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
