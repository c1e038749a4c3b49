#!/usr/bin/env python3
"""What the module-level autograd path costs against the fused train step, on configs/vfs_r18.py and configs/vfs_r50.py.

Two ways to take the same SimSiam step on one resident batch imgs [B,2,3,T,H,W] (default 8 x 2 x 3 x 4 x 224 x 224):
  loop  : as the reference writes it (sim_siam_base_tracker.py:31-56) - two backbone calls, two head calls, head.loss
          (CosineSimLoss in torch), loss.backward() through vfs_amd/autograd.py - eager launches, each view its own pass;
  fused : model.train_step + backward - both views stacked, recorded launch chains.
Both are followed by zero_grad and the optimizer step.  After `--warmup` steps, `--steps` steps are timed one by one with device
events (the host waits for each: the loop path is host-bound in places, and that is part of its cost); reported per path: median,
minimum and maximum ms per step over the timed steps, and the spread (max - min) / median.

Usage: python tools/bench_autograd_step.py [--batch 8] [--clip 4] [--size 224] [--steps 20] [--warmup 5] [--out FILE.json]"""
import json
import os
import statistics
import sys

import torch

REPO = __file__.rsplit('/tools/', 1)[0]
sys.path.insert(0, REPO)
import vfs_amd  # noqa: E402


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _model(cfg_name, dev):
    cfg = vfs_amd.Config.fromfile(os.path.join(REPO, 'configs', cfg_name))
    mcfg = dict(cfg.model)
    for part in ('backbone', 'img_head'):      # one process, one GPU: plain BatchNorm
        mcfg[part] = dict(mcfg[part], norm_cfg=dict(mcfg[part]['norm_cfg'], type='BN'))
    model = vfs_amd.build_model(mcfg, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg).to(dev).train()
    return model, vfs_amd.build_optimizer(model, cfg.optimizer)


def _timed(one, steps, warmup):
    for _ in range(warmup):
        loss = one()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = one()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    return dict(step_ms=med, min_ms=min(ms), max_ms=max(ms), spread=(max(ms) - min(ms)) / med, loss=float(loss))


def fused_step(cfg_name, imgs, steps, warmup):
    model, opt = _model(cfg_name, imgs.device)
    batch = dict(imgs=imgs, label=torch.zeros(imgs.shape[0], 1))

    def one():
        out = model.train_step(batch, None)
        opt.zero_grad()
        out['loss'].backward()
        opt.step()
        return out['loss'].detach()
    return _timed(one, steps, warmup)


def loop_step(cfg_name, imgs, steps, warmup):
    model, opt = _model(cfg_name, imgs.device)
    B, _, _, T, H, W = imgs.shape
    views = [imgs[:, v].transpose(1, 2).reshape(B * T, 3, H, W).contiguous() for v in range(2)]      # video2images per view
    bb, head = model.backbone, model.img_head

    def one():
        opt.zero_grad()
        x1, x2 = bb(views[0]), bb(views[1])
        (z1, p1), (z2, p2) = head(x1), head(x2)
        loss = sum(v.mean() for v in head.loss(p1, z1, p2, z2).values())      # _parse_losses: the mean of each loss
        loss.backward()
        opt.step()
        return loss.detach()
    return _timed(one, steps, warmup)


def main():
    B, T, size = _arg('--batch', 8), _arg('--clip', 4), _arg('--size', 224)
    steps, warmup = _arg('--steps', 20), _arg('--warmup', 5)
    dev = torch.device('cuda:0')
    imgs = torch.randn(B, 2, 3, T, size, size, generator=torch.Generator().manual_seed(0)).to(dev)
    res = dict(shape=list(imgs.shape), steps=steps, warmup=warmup, device=torch.cuda.get_device_name(0))
    for name, cfg in (('r18', 'vfs_r18.py'), ('r50', 'vfs_r50.py')):
        res[name] = dict(loop=loop_step(cfg, imgs, steps, warmup), fused=fused_step(cfg, imgs, steps, warmup))
        res[name]['loop_over_fused'] = res[name]['loop']['step_ms'] / res[name]['fused']['step_ms']
    print(json.dumps(res))
    if '--out' in sys.argv:
        out = _arg('--out', '')
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
