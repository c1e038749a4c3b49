#!/usr/bin/env python3
"""Train-step time of configs/vfs_r18_dense.py (ResNet-18 + DenseSimSiamHead) and of its loss kernels against their bytes moved.

Protocol: one resident batch imgs [B,2,3,T,H,W] (default 8 x 2 x 3 x 4 x 224 x 224: 32 frames per view, 7 x 7 positions of 512
channels), train_step + backward + the fused SGD step; after `--warmup` steps (the launch chains are recorded in them) `--steps`
steps are timed with device events around the whole loop.  The loss kernels are timed on their own on the step's p / z buffers
(events around `--repeats` back-to-back launches, the median of 5 such measurements); their algorithmic bytes: forward = the
four operands once per roll, 4 K Nv S C 2 bytes; backward = per view the p rows once, the z rows once per roll and the gradient
rows once, 2 (2 + K) Nv S C 2 bytes.  The frame-level config (configs/vfs_r18.py) runs in the same process under the same
protocol for scale.

Usage: python tools/bench_dense_head.py [--batch 8] [--clip 4] [--size 224] [--steps 20] [--warmup 5] [--repeats 50] [--out FILE.json]"""
import json
import os
import statistics
import sys

import torch

REPO = __file__.rsplit('/tools/', 1)[0]
sys.path.insert(0, REPO)
import vfs_amd  # noqa: E402
from vfs_amd.engine import BF16, shared_engine  # noqa: E402


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def step_time(cfg_name, imgs, steps, warmup):
    cfg = vfs_amd.Config.fromfile(os.path.join(REPO, 'configs', cfg_name))
    mcfg = dict(cfg.model)
    for part in ('backbone', 'img_head'):      # one process, one GPU: plain BatchNorm
        mcfg[part] = dict(mcfg[part], norm_cfg=dict(mcfg[part]['norm_cfg'], type='BN'))
    model = vfs_amd.build_model(mcfg, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).to(imgs.device).train()
    opt = vfs_amd.build_optimizer(model, cfg.optimizer)
    batch = dict(imgs=imgs, label=torch.zeros(imgs.shape[0], 1))

    def one():
        out = model.train_step(batch, None)
        opt.zero_grad()
        out['loss'].backward()
        opt.step()
        return out
    for _ in range(warmup):
        out = one()
    float(out['log_vars']['loss'])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        out = one()
    e1.record()
    torch.cuda.synchronize()
    return model, e0.elapsed_time(e1) / steps, float(out['log_vars']['loss'])


def loss_kernel_times(model, T, repeats):
    eng = shared_engine()
    c = model._gs.ctx
    p, z, Nv, K = c['p'], c['z'], c['Nv'], c['K']
    S, C = p.shape[1] * p.shape[2], p.shape[3]
    dev = p.device
    loss = torch.empty(K, Nv, device=dev)
    gl = torch.full((K, Nv), 1.0 / Nv, device=dev)
    dp = torch.empty(p.shape, dtype=BF16, device=dev)
    head = model.img_head

    def timed(fn):
        runs = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(repeats):
                fn()
            e1.record()
            torch.cuda.synchronize()
            runs.append(e0.elapsed_time(e1) * 1e3 / repeats)
        return statistics.median(runs)
    fwd = lambda: head.loss_fwd_nhwc(eng, p, z, loss, Nv, T, K, c['weight'])      # noqa: E731
    bwd = lambda: head.loss_bwd_nhwc(eng, p, z, gl, dp, Nv, T, K, c['weight'])      # noqa: E731
    fwd(), bwd()
    torch.cuda.synchronize()
    tf, tb = timed(fwd), timed(bwd)
    rows = Nv * S * C * 2.0
    bf, bb = 4 * K * rows, 2 * (2 + K) * rows
    return dict(Nv=Nv, S=S, C=C, K=K, fwd_us=tf, fwd_bytes=bf, fwd_GBps=bf / tf * 1e-3, bwd_us=tb, bwd_bytes=bb, bwd_GBps=bb / tb * 1e-3)


def main():
    B, T, size = _arg('--batch', 8), _arg('--clip', 4), _arg('--size', 224)
    steps, warmup, repeats = _arg('--steps', 20), _arg('--warmup', 5), _arg('--repeats', 50)
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    imgs = torch.randn(B, 2, 3, T, size, size, generator=g).to(dev)
    res = dict(shape=list(imgs.shape), steps=steps, warmup=warmup, device=torch.cuda.get_device_name(0))
    dense, ms, loss = step_time('vfs_r18_dense.py', imgs, steps, warmup)
    res['dense'] = dict(step_ms=ms, loss=loss, loss_kernels=loss_kernel_times(dense, T, repeats))
    del dense
    _, ms, loss = step_time('vfs_r18.py', imgs, steps, warmup)
    res['frame_level'] = dict(step_ms=ms, loss=loss)
    print(json.dumps(res))
    if '--out' in sys.argv:
        out = _arg('--out', '')
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
