#!/usr/bin/env python3
"""vfs_amd.masked_attention against the same function composed from torch ops on the GPU (tests/masked_attention_oracle.py:
einsum, masked_fill, topk, softmax, gather - it materialises the [N, T*HW, HW] scores and the window mask), forward alone and
forward + backward wrt query, key and value.

Shapes (N, C, T, H x W, CO, neighbor_range, topk; temperature 0.07, normalize):
    32, 1024, 2, 16 x 16, 3, 12, 10        the stage-4 map of a 256 x 256 frame pair
    32,  256, 2, 32 x 32, 3, 12, 10        the stage-2 map

One process.  Every GPU step (a warm-up or a timed loop of one path at one shape) runs under its own watchdog: a step that does
not finish within --step-timeout seconds ends the process with a traceback (faulthandler) - nothing is started on the GPU after
it.  After `--warmup` calls, `--steps` calls are timed one by one with device events; reported per path: median, minimum, maximum
ms and the spread (max - min) / median, and the largest difference between the two paths' outputs and gradients.

Usage: python tools/bench_masked_attention.py [--steps 20] [--warmup 5] [--step-timeout 60] [--out FILE.json]"""
import faulthandler
import json
import os
import statistics
import sys

import torch

REPO = __file__.rsplit('/tools/', 1)[0]
sys.path.insert(0, REPO)
import vfs_amd  # noqa: E402
from tests import masked_attention_oracle as MO  # noqa: E402

SHAPES = [(32, 1024, 2, 16, 16, 3, 12, 10), (32, 256, 2, 32, 32, 3, 12, 10)]
TEMPERATURE = 0.07


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


class watchdog:
    """the time limit of one GPU step"""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        print(f'[step] {self.what}', file=sys.stderr, flush=True)
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


def _timed(one, steps, warmup, limit, what):
    with watchdog(limit, what + ': warm-up'):
        for _ in range(warmup):
            one()
        torch.cuda.synchronize()
    ms = []
    with watchdog(limit, what + ': timed'):
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            one()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    return dict(ms=med, min_ms=min(ms), max_ms=max(ms), spread=(max(ms) - min(ms)) / med)


def bench_shape(shape, steps, warmup, limit, dev):
    N, C, T, H, W, CO, nr, topk = shape
    gen = torch.Generator().manual_seed(0)
    q, k, v, dout = (torch.randn(s, generator=gen).to(dev) for s in ((N, C, H, W), (N, C, T, H, W), (N, CO, T, H, W), (N, CO, H, W)))
    kw = dict(neighbor_range=nr, temperature=TEMPERATURE, topk=topk, normalize=True)
    res = dict(shape=dict(N=N, C=C, T=T, H=H, W=W, CO=CO, neighbor_range=nr, topk=topk, temperature=TEMPERATURE))
    grads = {}
    for name, fn in (('hip', vfs_amd.masked_attention), ('torch', MO.masked_attention)):
        ops = [t.clone().requires_grad_() for t in (q, k, v)]

        def fwd():
            with torch.no_grad():
                return fn(q, k, v, **kw)

        def fwd_bwd():
            for t in ops:
                t.grad = None
            out = fn(*ops, **kw)
            out.backward(dout)
            return out
        what = f'{name} {N}x{C}x{T}x{H}x{W}'
        res[name] = dict(forward=_timed(fwd, steps, warmup, limit, what + ' forward'),
                         forward_backward=_timed(fwd_bwd, steps, warmup, limit, what + ' forward + backward'))
        with watchdog(limit, what + ': results'):
            grads[name] = [fwd_bwd().detach()] + [t.grad.clone() for t in ops]
            torch.cuda.synchronize()
    res['max_abs_diff'] = {n: float((a - b).abs().max()) for n, a, b in zip(('out', 'dq', 'dk', 'dv'), grads['hip'], grads['torch'])}
    for part in ('forward', 'forward_backward'):
        res[f'torch_over_hip_{part}'] = res['torch'][part]['ms'] / res['hip'][part]['ms']
    return res


def main():
    steps, warmup, limit = _arg('--steps', 20), _arg('--warmup', 5), _arg('--step-timeout', 60)
    dev = torch.device('cuda:0')
    res = dict(steps=steps, warmup=warmup, device=torch.cuda.get_device_name(0), shapes=[bench_shape(s, steps, warmup, limit, dev) for s in SHAPES])
    print(json.dumps(res))
    if '--out' in sys.argv:
        out = _arg('--out', '')
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
