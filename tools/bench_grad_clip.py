#!/usr/bin/env python3
"""What gradient clipping costs on the fused train step (optimizer_config = dict(grad_clip=...), configs/r*_*.py:136).

For configs/vfs_r50.py and configs/vfs_r18.py at the bench batch (32 videos, 256 x 256, the config's clip_len), one model and one
resident batch per config, three ways to run the optimizer part of the step:
  (a) none   grad_clip=None: the step as bench.py times it;
  (b) fused  grad_clip=dict(max_norm=...): reduction over the gradient arena + finish + the clipped update, no host read;
  (c) torch  torch.nn.utils.clip_grad_norm_ over the trainable parameter views, float() of the norm (what mmcv's OptimizerHook
             logs), then the unclipped fused update - what a user of this package had before (b) existed.
Every step also reads the loss from the log values, as bench.py's does.  After `--warmup` steps per variant (the launch chains
are recorded in the first of them), `--repeats` rounds are timed; a round times `--steps` steps of (a), then (b), then (c), each
with a host clock around a loop that ends in a device synchronise, so drift of the shared machine hits all three alike.  Reported:
the median over the rounds, every round's value, the differences (b) - (a) and (c) - (a), and the bytes of the trainable
gradient ranges (one pass over them is what (b) adds).

Usage: python tools/bench_grad_clip.py [--models r50,r18] [--batch 32] [--size 256] [--steps 20] [--warmup 5] [--repeats 5] [--out FILE.json]"""
import json
import os
import statistics
import sys
import time

import torch

REPO = __file__.rsplit('/tools/', 1)[0]
sys.path.insert(0, REPO)
import vfs_amd  # noqa: E402


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def bench_config(depth, B, size, steps, warmup, repeats, max_norm, dev):
    cfg = vfs_amd.Config.fromfile(os.path.join(REPO, 'configs', f'vfs_r{depth}.py'))
    torch.manual_seed(0)
    model = vfs_amd.build_model(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).to(dev).train()
    model.flatten_parameters()
    imgs = torch.randn(B, 2, 3, int(cfg.clip_len), size, size, device=dev, generator=torch.Generator(device=dev).manual_seed(1234))
    batch = dict(imgs=imgs, label=torch.zeros(B, 1, device=dev))
    opts = dict(none=vfs_amd.build_optimizer(model, cfg.optimizer, optimizer_config=dict(grad_clip=None)),
                fused=vfs_amd.build_optimizer(model, cfg.optimizer, optimizer_config=dict(grad_clip=dict(max_norm=max_norm))),
                torch=vfs_amd.build_optimizer(model, cfg.optimizer))
    trainable = [p for p in model.parameters() if p.requires_grad]
    norms = {}

    def step(kind):
        opt = opts[kind]
        out = model.train_step(batch, opt)
        opt.zero_grad()
        out['loss'].backward()
        if kind == 'torch':
            norms[kind] = float(torch.nn.utils.clip_grad_norm_(trainable, max_norm))
        opt.step()
        out['log_vars']['loss']
        return out

    def timed(kind, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step(kind)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for kind in opts:
        for _ in range(warmup):
            step(kind)
    torch.cuda.synchronize()
    runs = {k: [] for k in opts}
    for _ in range(repeats):
        for kind in opts:
            runs[kind].append(timed(kind, steps))
    norms['fused'] = opts['fused'].last_grad_norm()
    segs = opts['fused']._arena()[1]
    med = {k: statistics.median(v) for k, v in runs.items()}
    return dict(model=f'r{depth}', imgs=list(imgs.shape), views=len(trainable), segments=len(segs),
                gradient_bytes=4 * sum(hi - lo for lo, hi in segs), max_norm=max_norm, last_norm=norms,
                step_ms=med, rounds_ms=runs, fused_minus_none_ms=med['fused'] - med['none'], torch_minus_none_ms=med['torch'] - med['none'])


def main():
    B, size = _arg('--batch', 32), _arg('--size', 256)
    steps, warmup, repeats = _arg('--steps', 20), _arg('--warmup', 5), _arg('--repeats', 5)
    dev = torch.device('cuda:0')
    res = dict(steps=steps, warmup=warmup, repeats=repeats, device=torch.cuda.get_device_name(0), configs=[])
    for m in _arg('--models', 'r50,r18').split(','):
        res['configs'].append(bench_config(int(m[1:]), B, size, steps, warmup, repeats, _arg('--max-norm', 1.0), dev))
        print(json.dumps(res['configs'][-1]), flush=True)
        from vfs_amd import engine
        engine._ENGINES.clear()
        torch.cuda.empty_cache()
    if '--out' in sys.argv:
        out = _arg('--out', '')
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
